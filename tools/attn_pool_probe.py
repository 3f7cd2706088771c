"""Time ov_attn_pool / ov_attn_pool_backward against the self-attention pair at a comparable FLOP count.

    python tools/attn_pool_probe.py [--iters 30] [--warmup 5]

Per shape: the median of `iters` event-timed calls after `warmup`, forward and backward, with the K | V bytes the forward must read
set against the device's HBM bandwidth.  The yardstick is ov_attention_lse + ov_attention_backward_saved at B = 256, L = 257, H = 12,
hd = 64 in the same process."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from openvision_amd import _lib                                  # noqa: E402
from openvision_amd._lib import check, ptr, stream_ptr           # noqa: E402

DEV = "cuda:0"
HBM_TBS = 6.3          # MI355X achievable copy bandwidth, TB/s (8.0 peak)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def pool(lib, B, L, nq, H, hd, iters, warmup):
    E = H * hd
    g = torch.Generator(device=DEV).manual_seed(0)
    q = torch.randn(nq, E, device=DEV, generator=g).to(torch.bfloat16)
    kv = torch.randn(B * L, 2 * E, device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn(B * nq, E, device=DEV, generator=g).to(torch.bfloat16)
    out = torch.empty(B * nq, E, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B * H, (nq + 31) // 32 * 32, dtype=torch.float32, device=DEV)
    dq = torch.empty(nq, E, dtype=torch.float32, device=DEV)
    dkv = torch.empty_like(kv)
    nb = lib.ov_attn_pool_backward_workspace_bytes(B, L, nq, H, hd)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    st = stream_ptr()
    fwd = lambda: check(lib.ov_attn_pool(ptr(q), E, ptr(kv), 2 * E, ptr(out), E, ptr(lse), B, L, nq, H, hd, hd ** -0.5, st), "fwd")
    bwd = lambda: check(lib.ov_attn_pool_backward(ptr(q), E, ptr(kv), 2 * E, ptr(out), E, ptr(dout), E, ptr(lse), ptr(dq), E, ptr(dkv), 2 * E,
                                                  B, L, nq, H, hd, hd ** -0.5, ptr(ws), nb, st), "bwd")
    tf, tb = timed(fwd, iters, warmup), timed(bwd, iters, warmup)
    kv_ms = B * L * 2 * E * 2 / (HBM_TBS * 1e12) * 1e3
    flop = 4.0 * B * H * nq * L * hd
    print(f"attn_pool  B={B} L={L} n_q={nq} H={H} hd={hd}: fwd {tf:.3f} ms ({flop / tf / 1e9:.1f} TFLOP/s)  bwd {tb:.3f} ms  "
          f"K|V read at {HBM_TBS} TB/s {kv_ms:.3f} ms  bwd workspace {nb / 2 ** 20:.1f} MiB")
    return tf, tb


def self_attention(lib, B, L, H, hd, iters, warmup):
    D = H * hd
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn(B * L, 3 * D, device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn(B * L, D, device=DEV, generator=g).to(torch.bfloat16)
    out = torch.empty(B * L, D, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B * H, (L + 31) // 32 * 32, dtype=torch.float32, device=DEV)
    dqkv = torch.empty_like(qkv)
    nb = lib.ov_attention_backward_workspace_bytes(B, L, H, hd)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    st = stream_ptr()
    fwd = lambda: check(lib.ov_attention_lse(ptr(qkv), 3 * D, ptr(out), D, ptr(lse), B, L, H, hd, hd ** -0.5, st), "fwd")
    bwd = lambda: check(lib.ov_attention_backward_saved(ptr(qkv), 3 * D, ptr(out), D, ptr(dout), D, ptr(dqkv), 3 * D, ptr(lse), B, L, H, hd,
                                                        hd ** -0.5, ptr(ws), nb, st), "bwd")
    tf, tb = timed(fwd, iters, warmup), timed(bwd, iters, warmup)
    flop = 4.0 * B * H * L * L * hd
    print(f"self-attn  B={B} L={L} H={H} hd={hd}: fwd {tf:.3f} ms ({flop / tf / 1e9:.1f} TFLOP/s)  bwd {tb:.3f} ms")
    return tf, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    lib = _lib.load()
    print(torch.cuda.get_device_name(0))
    self_attention(lib, 256, 257, 12, 64, a.iters, a.warmup)
    for H, hd in ((8, 96), (12, 64)):
        pool(lib, 256, 257, 256, H, hd, a.iters, a.warmup)
        pool(lib, 256, 257, 1, H, hd, a.iters, a.warmup)


if __name__ == "__main__":
    main()
