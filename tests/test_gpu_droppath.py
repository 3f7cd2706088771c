"""GPU: stochastic depth on the training path (ov_tower_set_drop_path; droppath.hip; training.drop_path_table).

  * the two glue kernels alone, bit for bit against torch on the device, with a guard pattern behind their outputs;
  * the tower walk under fixed masks at width 128, 2 heads, MLP 256, 3 layers, B = 5, L in {3, 65}: identity without drops,
    pass-through of a fully dropped sample, fp64 (tests/droppath_restate.py), compaction, recomputation, frozen blocks, a causal
    prefix, chunked nodes;
  * end to end on vit-tiny-patch16-160 at B = 4: clip_forward and accumulated_step.

The fp64 comparison.  Metric: hipops.ratio (test_gpu_block_chain.py's) of a tensor against its fp64 restatement with the tensor's
largest |reference| as the bound, the worst tensor of each group (output, dx, the 36 parameter gradients).  Yardstick: the same
figure of the run with NO table on the same inputs (code that exists without this feature).  A run under a table may exceed it by
the largest scale of the table (a branch's rounding error is multiplied by it) times 1.5 for the two extra bf16 roundings of the
glue; the bound is never taken from the table run itself.  Both figures are printed."""
import functools

import pytest
import torch

import droppath_restate as R
import hipops as H
from openvision_amd import _lib, preset, synth, training
from openvision_amd._lib import check, ptr, stream_ptr
from openvision_amd.accumulate import ContrastiveAccumulator
from openvision_amd.loss import ClipLoss
from openvision_amd.model import Transformer, create_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A
SLACK = 1.5


# ---- the glue kernels alone -------------------------------------------------------------------------------------------------------------
NB = 5
MASKS = {"k1": [0, 0, 1, 0, 0], "all": [1, 1, 1, 1, 1], "ends_kept": [1, 0, 1, 0, 1], "ends_dropped": [0, 1, 1, 1, 0]}


def _tables(mask):
    t = training.DropPathTable(torch.tensor(mask, dtype=torch.bool).view(1, 1, -1).expand(1, 2, -1).contiguous(), [1.0])
    idx, slot = t.host_tables()
    return idx[0, 0].to(DEV), slot[0, 0].to(DEV), t.counts[0][0]


def _guarded(rows, D):
    buf = torch.full((rows * D * 2 + 512,), GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[:rows * D * 2].view(torch.bfloat16).view(rows, D)


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("D", [64, 200])
@pytest.mark.parametrize("L", [1, 3, 65])
def test_glue_kernels_bitwise(L, D, mask):
    lib = _lib.load()
    idx, slot, k = _tables(MASKS[mask])
    g = torch.Generator().manual_seed(1000 * L + D)
    src = torch.randn(NB * L, D, generator=g).to(torch.bfloat16).to(DEV)
    kept = idx[:k].long()
    for scale in (1.0, 1.25, 1.0 / 0.7):
        buf, dst = _guarded(k * L, D)
        check(lib.ov_sample_gather(ptr(src), ptr(idx), ptr(dst), NB, k, L, D, scale, stream_ptr()), "ov_sample_gather")
        rows = src.view(NB, L, D)[kept].reshape(k * L, D)
        want = rows if scale == 1.0 else (rows.float() * scale).to(torch.bfloat16)
        assert H.same_bits(dst, want), ("gather", L, D, mask, scale)
        assert bool((buf[k * L * D * 2:] == GUARD).all()), "ov_sample_gather wrote past its last row"
    y = torch.randn(k * L, D, generator=g).to(torch.bfloat16).to(DEV)
    res = torch.randn(NB * L, D, generator=g).to(torch.bfloat16).to(DEV)
    keepb = (slot >= 0)
    for scale in (1.0, 1.0 / 0.7):
        want = res.clone().view(NB, L, D)
        want[keepb] = (res.view(NB, L, D)[keepb].float() + y.view(k, L, D)[slot[keepb].long()].float() * scale).to(torch.bfloat16)
        for alias in (False, True):
            buf, out = _guarded(NB * L, D)
            if alias:
                out.copy_(res)
            check(lib.ov_sample_scatter_axpy(ptr(out if alias else res), ptr(y), ptr(slot), ptr(out), NB, k, L, D, scale, stream_ptr()),
                  "ov_sample_scatter_axpy")
            assert H.same_bits(out, want.view(NB * L, D)), ("scatter", L, D, mask, scale, alias)
            assert H.same_bits(out.view(NB, L, D)[~keepb], res.view(NB, L, D)[~keepb]), "a dropped sample's rows are not the residual's"
            assert bool((buf[NB * L * D * 2:] == GUARD).all()), "ov_sample_scatter_axpy wrote past its last row"


# ---- the tower walk -------------------------------------------------------------------------------------------------------------------
D, HEADS, LAYERS = 128, 2, 3
# sample 4 is dropped by every branch of every block; block 0's MLP keeps nobody, block 1's attention keeps one sample
KEEP_A = [[[1, 1, 1, 1, 0], [0, 0, 0, 0, 0]],
          [[0, 0, 1, 0, 0], [1, 1, 0, 1, 0]],
          [[1, 0, 1, 1, 0], [0, 1, 1, 1, 0]]]
# block 0 keeps everyone at a scale that is not 1; the first and the last sample are dropped somewhere and kept elsewhere
KEEP_B = [[[1, 1, 1, 1, 1], [1, 1, 1, 1, 1]],
          [[0, 1, 1, 1, 0], [1, 0, 0, 1, 1]],
          [[1, 1, 0, 1, 1], [0, 1, 1, 0, 1]]]
SCALES = [1.25, 1.5, 2.0]
# sample 4 dropped everywhere, everyone else kept
KEEP_C = [[[1, 1, 1, 1, 0], [1, 1, 1, 1, 0]]] * LAYERS


@functools.lru_cache(maxsize=None)
def _tower():
    """The stack, its parameters rounded to bf16 (what the kernels read is what the restatement reads)."""
    tr = Transformer(D, LAYERS, HEADS, 2.0)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in tr.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            elif n.endswith("ln_1.weight") or n.endswith("ln_2.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            p.copy_(p.to(torch.bfloat16).float())
    return tr.to(DEV).train()


@functools.lru_cache(maxsize=None)
def _inputs(L):
    g = torch.Generator().manual_seed(7 + L)
    x = torch.randn(NB, L, D, generator=g).to(torch.bfloat16).float()
    wout = (torch.randn(NB, L, D, generator=g) * 0.1).to(torch.bfloat16).float()
    return x.to(DEV), wout.to(DEV)


def _table(keep, scale=SCALES):
    return training.drop_path_table(_tower(), NB, keep=torch.tensor(keep, dtype=torch.bool), scale=scale)


def _step(x, wout, drop=None, remat=False, chunk=0, prefix=None, frozen=0, need_x=True):
    """(y, dx or None, {name: grad or None}) of loss = sum(tower(x) * wout) on the HIP path."""
    tr = _tower()
    prev = training.CHUNK_LAYERS[0]
    tr.grad_checkpointing = remat
    training.set_backward_chunk_layers(chunk)
    for i, blk in enumerate(tr.resblocks):
        blk.requires_grad_(i >= frozen)
    try:
        for p in tr.parameters():
            p.grad = None
        xx = x.clone().requires_grad_(need_x)
        y = training.tower_forward(tr, xx, prefix=prefix, drop=drop)
        (y.float() * wout).sum().backward()
        torch.cuda.synchronize()
    finally:
        training.set_backward_chunk_layers(prev)
        tr.grad_checkpointing = False
        tr.requires_grad_(True)
    return (y.detach().clone(), xx.grad.detach().clone() if need_x else None,
            {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in tr.named_parameters()})


def _same(a, b, what, names=None):
    assert torch.equal(a[0], b[0]), (what, "output")
    if a[1] is not None and b[1] is not None:
        assert torch.equal(a[1], b[1]), (what, "dx")
    for n in (names if names is not None else b[2]):
        assert a[2][n] is not None and b[2][n] is not None and torch.equal(a[2][n], b[2][n]), (what, n)


_MODULE_NAMES = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                 "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")


def _errors(got, x, wout, keep, scale, prefix=None, first=0, samples=None):
    """{"output" | "dx" | "grads": worst H.ratio against the fp64 restatement, bound = the reference tensor's largest magnitude}."""
    tr = _tower()
    params = [R.block_params(b) for b in tr.resblocks]
    xs, ws = (x, wout) if samples is None else (x[samples], wout[samples])
    y, dx, grads = R.tower_grads(xs.cpu(), params, ws.cpu(), None if keep is None else torch.tensor(keep), scale, HEADS, False, prefix,
                                 tr.resblocks[0].ln_1.eps)
    rel = lambda a, ref: H.ratio(a.cpu(), ref, ref.abs().max().expand_as(ref))[0]
    res = {"output": rel(got[0], y)}
    if got[1] is not None:
        res["dx"] = rel(got[1], dx)
    res["grads"] = max(rel(got[2][f"resblocks.{i}.{m}"], grads[i][n]) for i in range(first, LAYERS) for n, m in zip(R.NAMES, _MODULE_NAMES))
    return res


@functools.lru_cache(maxsize=None)
def _yardstick(L, prefix=None):
    """The run with no table against fp64: (its results, its errors)."""
    x, wout = _inputs(L)
    plain = _step(x, wout, prefix=prefix)
    return plain, _errors(plain, x, wout, None, None, prefix)


def _within(tag, err, yard, max_scale):
    print(f"{tag}: " + "  ".join(f"{k} {err[k]:.3e} (no table {yard[k]:.3e}, bound {max_scale * SLACK * yard[k]:.3e})" for k in err))
    bad = {k: (err[k], yard[k]) for k in err if not err[k] <= max_scale * SLACK * yard[k]}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("L", [3, 65])
def test_no_drop_is_todays_path_bitwise(L):
    x, wout = _inputs(L)
    tr = _tower()
    plain, _ = _yardstick(L)
    assert tr.drop_path == 0.0 and tr.training
    _same(_step(x, wout, drop=None), plain, "rate 0")
    ones = [[[1] * NB] * 2] * LAYERS
    _same(_step(x, wout, drop=_table(ones, [1.0] * LAYERS)), plain, "all kept at scale 1")
    tr.set_drop_path(0.5)
    try:
        tr.eval()
        _same(_step(x, wout), plain, "eval mode draws nothing")
    finally:
        tr.train()
        tr.set_drop_path(0.0)


@pytest.mark.parametrize("L", [3, 65])
def test_fully_dropped_sample_passes_through(L):
    x, wout = _inputs(L)
    got = _step(x, wout, drop=_table(KEEP_A))
    assert torch.equal(got[0][4], x[4]), "the dropped sample's output rows are not its input rows"
    assert torch.equal(got[1][4], wout[4]), "the dropped sample's dx rows are not dy"
    assert not torch.equal(got[0][:4], x[:4])
    x2 = x.clone()
    x2[4] = (torch.randn(L, D, generator=torch.Generator().manual_seed(99)) * 3.0).to(torch.bfloat16).float().to(DEV)
    other = _step(x2, wout, drop=_table(KEEP_A))
    assert torch.equal(other[0][:4], got[0][:4]) and torch.equal(other[1][:4], got[1][:4])
    assert torch.equal(other[0][4], x2[4])
    for n in got[2]:
        assert torch.equal(other[2][n], got[2][n]), n
    for n in ("mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias"):
        assert not bool(got[2]["resblocks.0." + n].any()), ("a branch nobody kept has a gradient", n)


@pytest.mark.parametrize("table", ["A", "B"])
@pytest.mark.parametrize("L", [3, 65])
def test_against_fp64(L, table):
    x, wout = _inputs(L)
    keep = KEEP_A if table == "A" else KEEP_B
    got = _step(x, wout, drop=_table(keep))
    _, yard = _yardstick(L)
    _within(f"drop path vs fp64, L = {L}, table {table}", _errors(got, x, wout, keep, SCALES), yard, max(SCALES))


@pytest.mark.parametrize("L", [3, 65])
def test_compaction_equals_the_plain_run_on_the_kept_samples(L):
    x, wout = _inputs(L)
    got = _step(x, wout, drop=_table(KEEP_C, [1.0] * LAYERS))
    four = _step(x[:4].contiguous(), wout[:4].contiguous())
    _, yard = _yardstick(L)
    sub = (got[0][:4], got[1][:4], got[2])
    _within(f"compaction vs fp64, L = {L}", _errors(sub, x, wout, None, None, samples=slice(0, 4)), yard, 1.0)
    bitwise = torch.equal(sub[0], four[0]) and torch.equal(sub[1], four[1]) and all(torch.equal(sub[2][n], four[2][n]) for n in four[2])
    print(f"compaction, L = {L}: the four kept samples are {'bitwise' if bitwise else 'NOT bitwise'} the plain run on them")
    assert torch.equal(got[0][4], x[4]) and torch.equal(got[1][4], wout[4])


@pytest.mark.parametrize("L", [3, 65])
def test_recomputation_and_chunked_nodes_bitwise(L):
    x, wout = _inputs(L)
    for keep in (KEEP_A, KEEP_B):
        ref = _step(x, wout, drop=_table(keep))
        _same(_step(x, wout, drop=_table(keep), remat=True), ref, "recomputation")
        _same(_step(x, wout, drop=_table(keep), chunk=1), ref, "one node per block")
        _same(_step(x, wout, drop=_table(keep), remat=True, chunk=2), ref, "recomputation, two blocks per node")


@pytest.mark.parametrize("prefix", [None, 0])
@pytest.mark.parametrize("L", [3, 65])
def test_frozen_lower_blocks_and_prefix(L, prefix):
    x, wout = _inputs(L)
    top = [f"resblocks.2.{m}" for m in _MODULE_NAMES]
    _, yard = _yardstick(L, prefix)
    for keep in (KEEP_A, KEEP_B):
        full = _step(x, wout, drop=_table(keep), prefix=prefix)
        _within(f"all trainable, prefix {prefix}, L = {L}", _errors(full, x, wout, keep, SCALES, prefix), yard, max(SCALES))
        for remat in (False, True):
            part = _step(x, wout, drop=_table(keep), prefix=prefix, frozen=2, need_x=False, remat=remat)
            _same(part, full, ("first = 2", prefix, remat), names=top)
            assert all(part[2][f"resblocks.{i}.{m}"] is None for i in (0, 1) for m in _MODULE_NAMES)
        _within(f"first = 2, prefix {prefix}, L = {L}", _errors(part, x, wout, keep, SCALES, prefix, first=2), yard, max(SCALES))
        mid = _step(x, wout, drop=_table(keep), prefix=prefix, frozen=2, need_x=True)          # frozen blocks run input-only
        _same(mid, full, ("blocks 0, 1 frozen, dx wanted", prefix), names=top)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clip():
    cfg = preset("vit-tiny-patch16-160")
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    g = torch.Generator().manual_seed(21)
    size = m.visual.image_size[0]
    images = torch.randn(4, 3, size, size, generator=g).to(DEV)
    tokens = torch.randint(1, m.vocab_size - 1, (4, m.context_length), generator=g).to(DEV)
    return m, images, tokens


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_clip_forward_in_training_mode_is_repeatable_and_eval_is_untouched():
    m, images, tokens = _clip()
    m.eval()
    with torch.no_grad():
        base = [t.clone() for t in training.clip_forward(m, images, tokens)[:2]]
        inf = (m.encode_image(images, normalize=True).clone(), m.encode_text(tokens, normalize=True).clone())
    m.set_drop_path(image=0.3, text=0.3)
    try:
        with torch.no_grad():
            after = training.clip_forward(m, images, tokens)[:2]
            assert torch.equal(after[0], base[0]) and torch.equal(after[1], base[1]), "set_drop_path moved an eval model's features"
            assert torch.equal(m.encode_image(images, normalize=True), inf[0]) and torch.equal(m.encode_text(tokens, normalize=True), inf[1])
        m.train()
        runs = []
        for _ in range(2):
            torch.manual_seed(1234)
            m.zero_grad(set_to_none=True)
            img_f, txt_f, scale = training.clip_forward(m, images, tokens)[:3]
            ClipLoss()(img_f, txt_f, scale).backward()
            torch.cuda.synchronize()
            runs.append((img_f.detach().clone(), txt_f.detach().clone(), _grads(m)))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert runs[0][2].keys() == runs[1][2].keys() and len(runs[0][2]) > 20
        for n, g in runs[0][2].items():
            assert torch.equal(g, runs[1][2][n]), n
            assert bool(torch.isfinite(g).all()), n
        assert not torch.equal(runs[0][0], base[0]), "training mode at rate 0.3 dropped nothing (seed 1234 drops at B = 4)"
    finally:
        m.set_drop_path()
        m.eval()
        m.zero_grad(set_to_none=True)


def test_accumulated_step_uses_one_table_per_micro_batch_in_both_passes():
    m, images, tokens = _clip()
    m.set_drop_path(image=0.3, text=0.3)
    m.train()
    try:
        batches = [(images[:2], tokens[:2]), (images[2:], tokens[2:])]
        loss = ClipLoss()
        torch.manual_seed(77)
        m.zero_grad(set_to_none=True)
        total = training.accumulated_step(m, batches, loss, check=True)            # check: pass 2 reproduced pass 1's features bitwise
        torch.cuda.synchronize()
        got = _grads(m)
        assert bool(torch.isfinite(total))
        # the same two tables applied by hand: drawn in accumulated_step's order (per micro-batch: image tower, then text tower)
        torch.manual_seed(77)
        drops = [(training.drop_path_table(m.visual.transformer, 2), training.drop_path_table(m.transformer, 2)) for _ in batches]
        assert any(not bool(t.keep.all()) for pair in drops for t in pair)
        m.zero_grad(set_to_none=True)
        acc = ContrastiveAccumulator(loss)
        with torch.no_grad():
            for (im, tx), dr in zip(batches, drops):
                acc.add(*training.clip_forward(m, im, tx, drop=dr)[:2])
            want_total = acc.close(m.logit_scale.exp()).clone()
        for j, ((im, tx), dr) in enumerate(zip(batches, drops)):
            img_f, txt_f, scale = training.clip_forward(m, im, tx, drop=dr)[:3]
            acc.window_loss(j, img_f, txt_f, scale, check=True).backward()
        torch.cuda.synchronize()
        want = _grads(m)
        assert torch.equal(total, want_total)
        assert got.keys() == want.keys()
        for n in want:
            assert torch.equal(got[n], want[n]), n
    finally:
        m.set_drop_path()
        m.eval()
        m.zero_grad(set_to_none=True)
