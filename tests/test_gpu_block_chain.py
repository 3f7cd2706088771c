"""GPU: every stage of the training block chain held to its operator's fp64 bound in situ.

forward_saving_layer (tower.hip) and block_backward_chain (backward.hip) wire the operators together; the digests of
test_gpu_block_pinned.py and test_gpu_train_pinned.py anchor every variant of that wiring to the saving path bit for bit, and the
oracle tests of the chain (test_block_backward_vs_oracle, test_training_step_gradients_tiny) compare end results under tolerances that
twelve blocks of compounding bf16 error force: 4 % of a tensor's maximum cannot see an element that is 100 % wrong and thirty times
smaller than the largest.  Here each stage is checked against fp64 OF THAT STAGE ON ITS OWN INPUTS AS THE RUN PRODUCED THEM, under
the per-element bound its operator already has (hipops.chain_forward_ratios / chain_backward_ratios; what those checks tell apart is
pinned on the CPU by test_block_chain_cpu.py):

  * forward: a one-layer ov_tower_forward_saving, `saved` sliced by hipops.saved_slots into [x | qkv | o | x1 | ln_1 | ln_2 | pre |
    act | lse]: ln_1 of x, qkv of ln_1, attention (and the kept lse) of qkv, x1 of (o, x), ln_2 of x1, pre / act of ln_2 with columns
    [mlp, mlp_pad) exactly zero, y of (act, x1);
  * backward: hipops.block_chain_replay makes the chain's launches one by one through the operators the C ABI exports; every stage of
    the replay is inside its bound, and dx and the twelve gradients of ov_block_backward -- recomputing, over the full slot, and
    ov_block_backward_prefix at prefix L // 3 -- and of a one-layer ov_tower_backward are BITWISE the replay's: the claim backward.hip
    makes between its entry points, extended to the operators themselves;
  * the walk: a two- and a three-layer tower -- layer 0's slot holds the input, layer i + 1's holds what a one-layer tower of layer i
    makes of layer i's, every slot passes the forward table, and ov_tower_backward is bitwise the per-layer ov_block_backward(saved)
    calls made in reverse with dx handed down.

Shapes: the three rows of test_gpu_block_pinned.SHAPES (resident attention backward over the kept lse and the explicit-transpose dW;
streaming backward, tanh GELU and the TN dW route; head_dim 80 without a kept lse and mlp_pad > mlp).  x: hipops.spiked_rows_case;
dy: hipops.chain_dy, dense-and-spiked and pooled (non-zero on token 0 only; for the tanh block the mean pool's constant 1 / L on
tokens 1...).  Under the pooled dy the rows whose dy is zero are held to their bounds in dx1, dqkv and dx by name, and the ratio of
the largest to the smallest row norm of dx is printed.  Operands of the replay sit in NaN-padded buffers, its outputs start as SENT
in wider buffers whose padding must keep it, and every run is repeated bitwise."""
import functools

import pytest
import torch

import hipops as H
from hipops import BLOCK_NAMES, DEV, SENT
from test_gpu_block_pinned import SHAPES

pytestmark = pytest.mark.gpu
KINDS = ("dense", "pooled")
ROUTES = ("saved", "recompute", "prefix")
BWD_FORMS = {"hd64_l257": "resident saved", "hd64_l384_tanh": "stream<2>", "hd80_l257_padmlp": "stream<3>"}


def shape_of(tag, layers=1):
    D, heads, mlp, F, tanh, B, L, _ = SHAPES[tag]
    return (D, heads, mlp, F, tanh, B, L), H._lib.TowerCfg(D, layers, heads, mlp, F, int(tanh), 1e-6)


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """(block weights on the device, x, {kind: dy}): drawn once per shape and left unchanged."""
    (D, heads, mlp, F, tanh, B, L), _ = shape_of(tag)
    w = H.block_case(D, heads, mlp, B, L, tanh, 70, mlp_pad=F)[2]
    x = H.spiked_rows_case(B * L, D, seed=11)[0].to(DEV)
    return w, x, {k: H.chain_dy(k, B, L, D, tanh, seed=12).to(DEV) for k in KINDS}


def keeps_lse(dims):
    D, heads, _, _, _, B, L = dims
    return H.attn_route(B, L, heads, D // heads).keep_lse


def slot_tensors(slot, keep_lse):
    f = dict(slot)
    if not keep_lse:
        f["lse"] = None                   # the section is there, nothing writes it
    return f


def report(tag, res):
    print(f"{tag}: " + "  ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def outputs(dx, grads):
    return {"dx": dx, **{n: grads[n] for n in BLOCK_NAMES}}


def replay_outputs(r):
    return {"dx": r.dx.contiguous(), **{n: r.grads[n].contiguous() for n in BLOCK_NAMES}}


def test_shapes_reach_the_branches_they_are_here_for():
    """Host calls only: the kept lse at hd64_l257 alone, the TN dW route at B L % 64 == 0 alone, and the replay's operand pitches
    (8 columns wider) leave the attention kernel form where the dense call has it."""
    for tag in SHAPES:
        (D, heads, mlp, F, tanh, B, L), _ = shape_of(tag)
        hd = D // heads
        assert keeps_lse((D, heads, mlp, F, tanh, B, L)) == (tag == "hd64_l257")
        assert H.linear_backward_plan(B * L, 3 * D, D)[2] == (tag == "hd64_l384_tanh")
        for prefix in (None, L // 3):
            dense, wide = H.attn_route(B, L, heads, hd, prefix=prefix), H.attn_route(B, L, heads, hd, prefix=prefix, ld_qkv=3 * D + 8, ld_out=D + 8)
            assert (dense.form, dense.bwd_form) == (wide.form, wide.bwd_form), (tag, prefix)
        keep = tag == "hd64_l257"
        assert H.attn_route(B, L, heads, hd, lse=keep).bwd_form == BWD_FORMS[tag] and H.attn_route(B, L, heads, hd, prefix=L // 3).bwd_mask


@pytest.mark.parametrize("tag", list(SHAPES))
def test_forward_stages_out_of_saved(tag):
    dims, cfg = shape_of(tag)
    D, heads, mlp, F, tanh, B, L = dims
    w, x, _ = inputs(tag)
    with H.Tower(cfg, [w]) as t:
        y, saved = t.forward_saving(x, B, L)
        y2, saved2 = t.forward_saving(x, B, L)
    slot = H.saved_slots(saved, D, F, heads, B, L)[0]
    assert H.same_bits(slot["x"], x), "the slot's x is not the input"
    report(f"chain forward {tag}", H.chain_forward_ratios(w, slot_tensors(slot, keeps_lse(dims)), y, dims))
    assert H.same_bits(y, y2)
    nb = H.slot_layout(D, F, heads, B, L)[0]["lse"][0] if not keeps_lse(dims) else saved.numel()
    assert H.same_bits(saved[:nb], saved2[:nb])                         # (an unkept lse section is never written)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tag", list(SHAPES))
def test_backward_stages_and_entries_bitwise_the_replay(tag, route, kind):
    dims, cfg = shape_of(tag)
    D, heads, mlp, F, tanh, B, L = dims
    M = B * L
    w, x, dys = inputs(tag)
    dy = dys[kind]
    prefix = L // 3 if route == "prefix" else None
    entries = {}
    if route == "saved":
        with H.Tower(cfg, [w]) as t:
            _, saved = t.forward_saving(x, B, L)
            slot = H.saved_slots(saved, D, F, heads, B, L)[0]
            dx_t, grads_t = t.backward(saved, dy, B, L)
        entries["ov_tower_backward"] = outputs(dx_t, grads_t[0])
        entries["ov_block_backward(saved)"] = outputs(*H.block_backward(cfg, w, x, dy, B, L, saved=H.block_saved_of(slot, keeps_lse(dims))))
    else:
        slot = None
        name = "ov_block_backward(NULL)" if prefix is None else "ov_block_backward_prefix(NULL)"
        entries[name] = outputs(*H.block_backward(cfg, w, x, dy, B, L, prefix=prefix))
    r = H.block_chain_replay(cfg, w, x, slot, dy, B, L, prefix)
    again = H.block_chain_replay(cfg, w, x, slot, dy, B, L, prefix)
    torch.cuda.synchronize()

    tagline = f"chain backward {tag} {route} {kind}"
    if slot is None:                      # the replay's own forward, stage by stage (the kept one: test_forward_stages_out_of_saved)
        report(tagline + " (replayed forward)", H.chain_forward_ratios(w, r.f, None, dims, prefix))
    res, elem = H.chain_backward_ratios(w, r, dy, dims, prefix)
    report(tagline, res)
    for wide, cols in r.wides:
        assert bool((wide[:, cols:] == SENT).all()), (tagline, "an output's padding was written", tuple(wide.shape), cols)
    assert (r.dh_lin is None) == (route == "saved") and (r.f["lse"] is not None) == (route == "saved" and keeps_lse(dims))

    want = replay_outputs(r)
    assert not H.same_outputs(replay_outputs(again), want), (tagline, "the replay is not deterministic")
    for name, got in entries.items():
        differ = H.same_outputs(got, want)
        assert not differ, (tagline, name, "differs from the operator-by-operator replay in", differ)

    if kind == "pooled":                  # the rows that receive no dy: fed through dK and dV alone, far below the tensor's largest
        quiet = (dy.float().abs().amax(1) == 0).cpu()
        assert 0 < int(quiet.sum()) < M
        worst = {k: float(q[quiet].max()) for k, q in elem.items()}
        norms = r.dx.float().norm(dim=1).cpu()
        print(f"{tagline}: rows with dy = 0: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items())
              + f"; dx row norms: largest / smallest = {float(norms.max() / norms.min()):.3g}, largest / median row with dy = 0 = "
              f"{float(norms.max() / norms[quiet].median()):.3g}")
        assert all(v <= 1.0 for v in worst.values()), (tagline, worst)


@pytest.mark.parametrize("tag", ["hd64_l384_tanh", "hd64_l257"])
def test_tower_walk_is_the_block_entry_layer_by_layer(tag):
    layers = SHAPES[tag][7]
    dims, cfg = shape_of(tag, layers)
    D, heads, mlp, F, tanh, B, L = dims
    _, cfg1 = shape_of(tag)
    _, x, dys = inputs(tag)
    dy = dys["dense"]
    ws = [H.block_case(D, heads, mlp, B, L, tanh, 70 + 100 * i, mlp_pad=F)[2] for i in range(layers)]
    keep = keeps_lse(dims)
    with H.Tower(cfg, ws) as t:
        y, saved = t.forward_saving(x, B, L)
        slots = H.saved_slots(saved, D, F, heads, B, L, layers)
        dx, grads = t.backward(saved, dy, B, L)
    assert H.same_bits(slots[0]["x"], x), "layer 0's slot does not hold the input"
    names = H.SLOT_FIELDS + (("lse",) if keep else ())
    for i in range(layers):
        nxt = slots[i + 1]["x"] if i + 1 < layers else y
        with H.Tower(cfg1, [ws[i]]) as t1:                                # layer i alone, on layer i's kept input
            y1, saved1 = t1.forward_saving(slots[i]["x"].clone(), B, L)
        alone = H.saved_slots(saved1, D, F, heads, B, L)[0]
        assert H.same_bits(nxt, y1), (tag, i, "the next layer's input is not this layer's output")
        differ = H.same_outputs({k: slots[i][k] for k in names}, {k: alone[k] for k in names})
        assert not differ, (tag, i, "the walk's slot differs from the one-layer tower's in", differ)
        report(f"chain walk {tag} layer {i}", H.chain_forward_ratios(ws[i], slot_tensors(slots[i], keep), nxt, dims))
    d = dy
    for i in reversed(range(layers)):
        d, g = H.block_backward(cfg1, ws[i], slots[i]["x"], d, B, L, saved=H.block_saved_of(slots[i], keep))
        differ = H.same_outputs(grads[i], g)
        assert not differ, (tag, i, "ov_tower_backward differs from ov_block_backward(saved) in", differ)
    assert H.same_bits(dx, d), (tag, "dx of the walk differs from the per-layer calls'")
