"""CPU: the distillation loss (openvision_amd.loss.DistillClipLoss, reference open_clip/loss.py:180-216) -- the float64 restatement
against the reference class run over gloo (tests/golden/distill_grad.npz), the C ABI without a device, the module's refusals, and the
packed gather and the gradient routing over gloo."""
import os

import pytest
import torch

from openvision_amd import _lib
from openvision_amd import build as B
from openvision_amd import loss as L
from openvision_amd.loss import DistillClipLoss

import distill_restate as DR
from conftest import golden
from ranks import run_ranks

IDS = [c[0] for c in DR.CASES]
KEYS = ("img", "txt", "timg", "ttxt")


@pytest.fixture(scope="module")
def fixture():
    return golden("distill_grad.npz")


def fixture_case(z, case):
    """The case's inputs regenerated from their seed, checked against the fixture's sums."""
    name, ws, b, e, et, local_loss, gwg, s, st, seed = case
    inputs = DR.case_inputs(ws, b, e, et, seed)
    for key, x in zip(KEYS, inputs):
        ref_abs = float(z[f"{name}_{key}_abs_sum"])
        assert abs(float(x.sum()) - float(z[f"{name}_{key}_sum"])) <= 1e-9 * ref_abs, (name, key)
        assert abs(float(x.abs().sum()) - ref_abs) <= 1e-9 * ref_abs, (name, key)
    return inputs


def test_fixture_covers_the_cases(fixture):
    assert list(fixture["cases"]) == IDS and tuple(fixture["grads"]) == DR.GRADS == (1.0, 0.7)
    assert {c[1] for c in DR.CASES} == {1, 2, 3} and {c[2] for c in DR.CASES} == {13, 16}
    assert {(c[5], c[6]) for c in DR.CASES if c[1] > 1} == {(True, False), (True, True), (False, False)}
    assert {(c[3], c[4]) for c in DR.CASES} == {(64, 96), (64, 32), (768, 512)}
    assert all(c[7] == 5.0 and 10.0 <= c[8] <= 20.0 for c in DR.CASES)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "distill_grad.npz")) < 1 << 20


@pytest.mark.parametrize("case", DR.CASES, ids=IDS)
def test_the_teacher_matters_in_every_case(fixture, case):
    """The teacher's softmax is neither flat nor one-hot: in float64 the distill loss moves by >= 5 % when it is replaced by a
    uniform one and by the labels, on every rank; and the distill loss is not the contrastive loss."""
    name, ws, b, e, et, local_loss, gwg, s, st, seed = case
    inputs = fixture_case(fixture, case)
    for x in inputs:
        assert torch.allclose(x.norm(dim=-1), torch.ones(ws * b, dtype=torch.float64), atol=1e-6)
    for r in range(ws):
        args, off = DR.rank_args(inputs, r, ws, local_loss)
        c, d = (float(v) for v in DR.strip_losses(*args, s, st, off))
        rows, n = args[0].shape[0], args[2].shape[0]
        uniform = torch.full((rows, n), 1.0 / n, dtype=torch.float64)
        onehot = torch.zeros(rows, n, dtype=torch.float64)
        onehot[torch.arange(rows), torch.arange(rows) + off] = 1.0
        assert abs(float(DR.distill_under(uniform, uniform, *args[:4], s)) - d) >= 0.05 * d, (name, r)
        d_onehot = float(DR.distill_under(onehot, onehot, *args[:4], s))
        assert abs(d_onehot - d) >= 0.05 * d and abs(d_onehot - c) <= 1e-12 * c, (name, r)


@pytest.mark.parametrize("case", DR.CASES, ids=IDS)
def test_restatement_reproduces_the_reference(fixture, case):
    """Every rank's two losses and, for the upstream pair (1, 0.7), its gradients equal what the reference's DistillClipLoss gave by
    autograd over gloo, to 1e-12 relative: the losses and d logit_scale, which the fixture stores as float64, and the float64 sum and
    absolute sum of each feature gradient; the gradients' entries, which it stores as float32, to the rounding of that format."""
    name, ws, b, e, et, local_loss, gwg, s, st, seed = case
    inputs = fixture_case(fixture, case)
    per = DR.per_rank(inputs, s, st, ws, local_loss, gwg, *DR.GRADS)
    for r, (c, d, di, dt, ds) in enumerate(per):
        for got, key in ((c, "contrastive"), (d, "distill"), (ds, "dscale")):
            ref = float(fixture[f"{name}_{key}"][r])
            assert abs(float(got) - ref) <= 1e-12 * abs(ref), (name, r, key, float(got), ref)
        for got, key in ((di, "dimg"), (dt, "dtxt")):
            want = torch.from_numpy(fixture[f"{name}_{key}"][r]).double()
            assert got.shape == want.shape == (b, e), (name, key)
            assert float((got - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max()), (name, r, key)
            ref_abs = float(fixture[f"{name}_{key}_abs_sum"][r])
            assert abs(float(got.sum()) - float(fixture[f"{name}_{key}_sum"][r])) <= 1e-12 * ref_abs, (name, r, key)
            assert abs(float(got.abs().sum()) - ref_abs) <= 1e-12 * ref_abs, (name, r, key)


@pytest.mark.parametrize("case", DR.CASES, ids=IDS)
def test_autograd_of_the_restatement_equals_its_closed_form(case):
    name, ws, b, e, et, local_loss, gwg, s, st, seed = case
    inputs = DR.case_inputs(ws, b, e, et, seed)
    args, off = DR.rank_args(inputs, ws - 1, ws, True)
    leaves = [x.clone().requires_grad_(k < 4) for k, x in enumerate(args)]
    sc = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    c, d = DR.strip_losses(*leaves, sc, st, off)
    (0.3 * c + 2.0 * d).backward()
    closed = DR.strip_grads(*args, s, st, off, 0.3, 2.0)
    for x, want in zip(leaves[:4] + [sc], closed):
        assert torch.allclose(x.grad, torch.as_tensor(want), rtol=1e-10, atol=1e-14), name
    assert all(x.grad is None for x in leaves[4:])
    terms = DR.strip_terms(*args, s, st, off)
    c, d = c.detach(), d.detach()
    assert terms.shape == (8, b)
    assert abs(float((terms[0] - terms[1] + terms[2] - terms[3]).mean() / 2 - c)) < 1e-12
    assert abs(float((terms[0] - terms[5] + terms[2] - terms[7]).mean() / 2 - d)) < 1e-12


SYMS = ("ov_distill_loss_workspace_bytes", "ov_distill_loss", "ov_distill_loss_backward_workspace_bytes", "ov_distill_loss_backward")


def test_new_symbols_exported_bound_and_validating():
    lib = _lib.load()
    for s in SYMS:
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert lib.ov_abi_version() == 2 and "distill.hip" in B.SOURCES
    wsz, bsz = lib.ov_distill_loss_workspace_bytes, lib.ov_distill_loss_backward_workspace_bytes
    assert wsz(256, 2048) > lib.ov_clip_loss_workspace_bytes(256, 2048) > 0
    assert wsz(0, 64) == 0 and wsz(16, 0) == 0 and wsz(16, -4) == 0
    assert bsz(4096, 32768) >= 2 * 128 * 4 and bsz(0, 64) == 0 and bsz(16, 0) == 0 and bsz(-1, 64) == 0
    fake = 1 << 20                                   # never dereferenced: every call below fails its checks first
    ws = wsz(16, 64)

    def fwd(i=fake, t=fake, ai=fake, at=fake, ld=224, ti=fake, tt=fake, tai=fake, tat=fake, ldt=224, b=16, n=64, e=64, et=48, s=fake,
            st=fake, off=0, c=fake, d=fake, terms=fake, w=fake, wb=ws):
        return lib.ov_distill_loss(i, t, ai, at, ld, ti, tt, tai, tat, ldt, b, n, e, et, s, st, off, c, d, terms, w, wb, None)

    for k in ("i", "t", "ai", "at", "ti", "tt", "tai", "tat", "s", "st", "c", "d", "terms", "w"):
        assert fwd(**{k: None}) == -1, k
    assert fwd(b=0) == -1 and fwd(n=0) == -1 and fwd(b=65) == -1 and fwd(e=0) == -1 and fwd(et=0) == -1
    assert fwd(off=-1) == -1 and fwd(off=49) == -1
    assert fwd(e=40, ld=40) == -2 and fwd(e=1152 + 32, ld=1184) == -2 and fwd(et=36) == -2           # E % 32, E <= 1152, Et % 8
    assert fwd(ld=60) == -1 and fwd(ld=226) == -1 and fwd(ldt=40) == -1 and fwd(ldt=50) == -1       # pitch rules
    for k in ("i", "t", "ai", "at", "ti", "tt", "tai", "tat", "w"):
        assert fwd(**{k: fake + 4}) == -1, k         # 16-byte alignment
    assert fwd(wb=ws - 1) == -3
    wsb = bsz(16, 64)

    def bwd(i=fake, t=fake, ai=fake, at=fake, ld=224, ti=fake, tt=fake, tai=fake, tat=fake, ldt=224, b=16, n=64, e=64, et=48, s=fake,
            st=fake, off=0, terms=fake, gc=fake, gd=fake, di=fake, dt=fake, dai=None, dat=None, ldg=0, w=fake, wb=wsb):
        return lib.ov_distill_loss_backward(i, t, ai, at, ld, ti, tt, tai, tat, ldt, b, n, e, et, s, st, off, terms, gc, gd, di, dt, dai,
                                            dat, ldg, None, w, wb, None)

    for k in ("i", "t", "ai", "at", "ti", "tt", "tai", "tat", "s", "st", "terms", "gc", "gd", "di", "dt", "w"):
        assert bwd(**{k: None}) == -1, k             # both upstream gradients are required
    assert bwd(b=-1) == -1 and bwd(b=65) == -1 and bwd(off=60) == -1
    assert bwd(e=40, ld=40) == -2 and bwd(e=1152 + 32, ld=1184) == -2 and bwd(et=36) == -2
    assert bwd(ld=32) == -1 and bwd(ldt=44) == -1
    assert bwd(dai=fake, dat=fake, ldg=60) == -1 and bwd(dai=fake, dat=fake, ldg=130) == -1
    assert bwd(dai=fake + 8, dat=fake, ldg=128) == -1 and bwd(di=fake + 4) == -1
    assert bwd(wb=wsb - 1) == -3 and bwd(dai=fake, dat=fake, ldg=128, wb=wsb - 1) == -3


def test_loss_module_refusals_and_surface():
    import openvision_amd
    assert openvision_amd.DistillClipLoss is DistillClipLoss and "DistillClipLoss" in openvision_amd.__all__
    with pytest.raises(NotImplementedError):
        DistillClipLoss(use_horovod=True)
    fn = DistillClipLoss(local_loss=True, gather_with_grad=True, rank=1, world_size=2, group=None)
    assert (fn.local_loss, fn.gather_with_grad, fn.rank, fn.world_size, fn.always_collective, fn.last_terms) == (True, True, 1, 2, False, None)
    nrm = torch.nn.functional.normalize
    img, txt = nrm(torch.randn(4, 32), dim=-1), nrm(torch.randn(4, 32), dim=-1)
    t_img, t_txt = nrm(torch.randn(4, 16), dim=-1), nrm(torch.randn(4, 16), dim=-1)
    with pytest.raises(_lib.OvhipError):                            # CPU tensors: no eager fallback
        DistillClipLoss()(img, txt, torch.tensor(10.0), t_img, t_txt, torch.tensor(20.0))
    with pytest.raises(_lib.OvhipError):
        DistillClipLoss()(img.clone().requires_grad_(True), txt, 10.0, t_img, t_txt, 20.0)
    # a teacher that asks for a gradient is refused, whichever of its three inputs does
    for k in range(3):
        teacher = [t_img.clone(), t_txt.clone(), torch.tensor(20.0)]
        teacher[k].requires_grad_(True)
        with pytest.raises(ValueError, match="frozen"):
            DistillClipLoss()(img.clone().requires_grad_(True), txt, torch.tensor(10.0), *teacher)
    # shapes
    with pytest.raises(ValueError):
        DistillClipLoss()(img, txt[:3], 10.0, t_img, t_txt, 20.0)               # student sides differ
    with pytest.raises(ValueError):
        DistillClipLoss()(img, txt, 10.0, t_img, t_txt[:, :8], 20.0)            # teacher sides differ
    with pytest.raises(ValueError):
        DistillClipLoss()(img, txt, 10.0, t_img[:3], t_txt[:3], 20.0)           # teacher batch differs from the student's
    with pytest.raises(ValueError):
        DistillClipLoss()(img[0], txt[0], 10.0, t_img, t_txt, 20.0)             # not 2-d


def _gloo_rank(rank, ws):
    b, e, et = 3, 8, 4
    log = []
    L.record_comm(log)
    rows = torch.arange(b)[:, None].float()
    feats = [torch.full((b, w), 100.0 * rank + 10.0 * k) + rows for k, w in enumerate((e, e, et, et))]   # value = 100 rank + 10 k + row
    packed = L.gather_distill_features(*feats, ws)
    L.record_comm(None)
    # a hand-made packed [N, 2E] gradient of the student's gathered rows that differs on every rank
    g = torch.Generator().manual_seed(9)
    fulls = [torch.randn(ws * b, 2 * e, generator=g) for _ in range(ws)]
    summed = L.route_packed_gradient(fulls[rank].clone(), b, rank, True)
    own = L.route_packed_gradient(fulls[rank].clone(), b, rank, False)
    return packed, len(log), summed.clone(), own.clone(), fulls


def test_packed_gather_and_gradient_routing_over_gloo():
    """Two gloo ranks on CPU tensors: ONE collective gathers the packed [b, 2E + 2Et] rows in rank order, the columns split into the
    four operands, and a packed [N, 2E] gradient of the student's gathered rows is routed as each mode prescribes."""
    ws, b, e, et = 2, 3, 8, 4
    res = run_ranks(_gloo_rank, ws, timeout=300, backend="gloo")
    for rank in range(ws):
        packed, ncoll, summed, own, fulls = res[rank]
        assert ncoll == 1 and packed.shape == (ws * b, 2 * e + 2 * et)
        views = L.unpack_distill_features(packed, e)
        assert [tuple(v.shape) for v in views] == [(ws * b, e), (ws * b, e), (ws * b, et), (ws * b, et)]
        for g in range(ws * b):                                                           # rank order, row order
            for k, v in enumerate(views):
                assert torch.all(v[g] == 100.0 * (g // b) + 10.0 * k + g % b)
        assert views[1].data_ptr() == packed.data_ptr() + 4 * e and views[3].data_ptr() == packed.data_ptr() + 4 * (2 * e + et)
        assert torch.allclose(summed, sum(fulls)[rank * b:(rank + 1) * b])
        assert torch.equal(own, fulls[rank][rank * b:(rank + 1) * b])
    # pack / unpack are inverses on a local batch
    feats = [torch.randn(b, w) for w in (e, e, et, et)]
    for x, y in zip(L.unpack_distill_features(L.pack_distill_features(*feats), e), feats):
        assert torch.equal(x, y)
