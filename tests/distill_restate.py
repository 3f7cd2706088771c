"""Host-side float64 torch restatement of the reference's ``DistillClipLoss`` (open_clip/loss.py:180-216) on local logit strips, with
its gradients in closed form and the routing of the gathered side per rank (gather_features, loss.py:19-63).  What pins it numerically
is the reference class itself, run in float64 over gloo (tests/golden/distill_grad.npz, made by tests/golden/make_golden_distill.py);
tests/test_distill_cpu.py checks the restatement against that fixture before any kernel runs.

Also: the fixture's cases and their inputs, regenerated from recorded seeds (the fixture stores checksums, not the inputs)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

# name, world_size, b (rows per rank), E (student), Et (teacher), local_loss, gather_with_grad, s, st (the two multipliers), seed.
# s = 5 keeps the student's loss of order 1 (the 1e-5 RELATIVE bound on a loss is then a statement about lse - diag and not about its
# cancellation); st = 10 ... 20 gives a teacher softmax that is neither flat nor one-hot (make_golden_distill.py asserts that the
# distill loss moves by >= 5 % under either replacement, so a kernel that drops or mis-normalises Q cannot pass).
CASES = [
    ("ws1_b13_e64_t96", 1, 13, 64, 96, True, False, 5.0, 10.0, 301),
    ("ws1_b16_e64_t32", 1, 16, 64, 32, False, False, 5.0, 12.0, 302),
    ("ws2_b13_e64_t96_local", 2, 13, 64, 96, True, False, 5.0, 15.0, 303),
    ("ws2_b16_e64_t32_local_gwg", 2, 16, 64, 32, True, True, 5.0, 10.0, 304),
    ("ws3_b13_e64_t32_global", 3, 13, 64, 32, False, False, 5.0, 16.0, 305),
    ("ws3_b16_e64_t96_local_gwg", 3, 16, 64, 96, True, True, 5.0, 20.0, 306),
    ("ws2_b16_e64_t96_global", 2, 16, 64, 96, False, False, 5.0, 10.0, 307),
    ("ws2_b13_e768_t512_local_gwg", 2, 13, 768, 512, True, True, 5.0, 14.0, 308),
    ("ws3_b16_e768_t512_local", 3, 16, 768, 512, True, False, 5.0, 10.0, 309),
]

GRADS = (1.0, 0.7)          # the upstream pair (g_c, g_d) of the fixture's gradients

N_CENTRES, LATENT, SPREAD, NOISE_STUDENT, NOISE_TEACHER = 5, 8, 0.7, 1.0, 0.5


def make_inputs(n: int, e: int, et: int, seed: int, dtype=torch.float64):
    """(img, txt, t_img, t_txt): student [n, E] and teacher [n, Et] embeddings of n pairs, L2-normalised in fp32 and returned as
    ``dtype`` holding fp32 values.  The pairs share a clustered latent (5 centres in 8 dimensions, spread 0.7 round the centre): pairs
    of one cluster are near-duplicates, which is what a teacher's soft targets are about.  Each model has ONE random projection of
    the latent (image and text of a model live in one space) and each side its own noise
    vector (of norm about 1.0 for the student and 0.5 for the teacher, against a projected latent of norm about 3: the teacher is the
    sharper model)."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(N_CENTRES, LATENT, generator=g)
    z = centres[torch.randint(0, N_CENTRES, (n,), generator=g)] + SPREAD * torch.randn(n, LATENT, generator=g)
    out = []
    for width, noise in ((e, NOISE_STUDENT), (et, NOISE_TEACHER)):
        proj = torch.randn(LATENT, width, generator=g) / width ** 0.5
        for _ in range(2):
            out.append(F.normalize(z @ proj + noise * torch.randn(n, width, generator=g) / width ** 0.5, dim=-1))
    return tuple(t.to(dtype) for t in out)


def case_inputs(ws: int, b: int, e: int, et: int, seed: int):
    """The global sets of a case: rank r owns rows [r b, (r + 1) b) of all four."""
    return make_inputs(ws * b, e, et, seed)


def dist_loss(teacher_logits, student_logits):
    return -(teacher_logits.softmax(dim=1) * student_logits.log_softmax(dim=1)).sum(dim=1).mean(dim=0)      # loss.py:182-183


def strip_losses(x_img, x_txt, y_img, y_txt, u_img, u_txt, v_img, v_txt, s, st, off: int):
    """loss.py:185-216 on this rank's strips: local rows x / u against gathered sets y / v, labels i + off."""
    logits_per_image, logits_per_text = s * x_img @ y_txt.T, s * x_txt @ y_img.T                           # :195-196 (:108-110)
    dist_logits_per_image, dist_logits_per_text = st * u_img @ v_txt.T, st * u_txt @ v_img.T              # :198-199
    labels = torch.arange(x_img.shape[0], device=x_img.device) + off                                      # :201 (:92-94)
    contrastive = (F.cross_entropy(logits_per_image, labels) + F.cross_entropy(logits_per_text, labels)) / 2        # :203-206
    distill = (dist_loss(dist_logits_per_image, logits_per_image) + dist_loss(dist_logits_per_text, logits_per_text)) / 2   # :208-211
    return contrastive, distill


def distill_under(q_img, q_txt, x_img, x_txt, y_img, y_txt, s):
    """The distill loss with the teacher's two softmax matrices replaced by ``q_img`` / ``q_txt`` (rows summing to one)."""
    li, lt = torch.log_softmax(s * x_img @ y_txt.T, 1), torch.log_softmax(s * x_txt @ y_img.T, 1)
    return (-(q_img * li).sum(1).mean() - (q_txt * lt).sum(1).mean()) / 2


def strip_terms(x_img, x_txt, y_img, y_txt, u_img, u_txt, v_img, v_txt, s, st, off: int):
    """[8, b]: the first eight rows of what ov_distill_loss writes as ``terms`` (rows 8 ... 11 are the fp32 low parts of the four
    lse, whose high parts are rows 0, 2, 4, 6): the student's lse_img, diag_img, lse_txt, diag_txt, then per direction the
    teacher's lse and the cross sum sum_j Q_ij A_ij."""
    idx = torch.arange(x_img.shape[0], device=x_img.device)
    a, bt = s * x_img @ y_txt.T, s * x_txt @ y_img.T
    t, ut = st * u_img @ v_txt.T, st * u_txt @ v_img.T
    return torch.stack([torch.logsumexp(a, 1), a[idx, idx + off], torch.logsumexp(bt, 1), bt[idx, idx + off],
                        torch.logsumexp(t, 1), (torch.softmax(t, 1) * a).sum(1), torch.logsumexp(ut, 1), (torch.softmax(ut, 1) * bt).sum(1)])


def strip_grads_weighted(x_img, x_txt, y_img, y_txt, u_img, u_txt, v_img, v_txt, s, st, off: int, w_p: float, w_1: float, w_q: float):
    """The student-side gradients for the coefficient G = (w_p P - w_1 onehot - w_q Q) / (2 b) per direction, P = softmax(A),
    Q = softmax(T):  d x = s G y,  d y = s G^T x,  d s = sum G .* (x y^T).  (w_p, w_1, w_q) = (1, 0, 0) is the gradient of the mean
    lse, (0, -1, 0) of the mean label logit, (0, 0, -1) of the mean cross sum.  Returns (d_x_img, d_x_txt, d_y_img, d_y_txt, d_s)."""
    b = x_img.shape[0]
    idx = torch.arange(b, device=x_img.device)

    def coef(dots, tdots):
        g = w_p * torch.softmax(s * dots, 1) - w_q * torch.softmax(st * tdots, 1)
        g[idx, idx + off] -= w_1
        return g / (2 * b)

    di, dt = x_img @ y_txt.T, x_txt @ y_img.T
    gi, gt = coef(di, u_img @ v_txt.T), coef(dt, u_txt @ v_img.T)
    return s * gi @ y_txt, s * gt @ y_img, s * gt.T @ x_txt, s * gi.T @ x_img, (gi * di).sum() + (gt * dt).sum()


def strip_grads(x_img, x_txt, y_img, y_txt, u_img, u_txt, v_img, v_txt, s, st, off: int, g_c: float = 1.0, g_d: float = 1.0):
    """Closed form of the gradient of g_c contrastive + g_d distill, every student argument an independent leaf:
    G = ((g_c + g_d) P - g_c onehot - g_d Q) / (2 b).  Returns (d_x_img, d_x_txt, d_y_img, d_y_txt, d_s)."""
    return strip_grads_weighted(x_img, x_txt, y_img, y_txt, u_img, u_txt, v_img, v_txt, s, st, off, g_c + g_d, g_c, g_d)


def rank_args(inputs, r: int, ws: int, local_loss: bool):
    """The eight operands and the label offset of rank r: its own rows against the global sets, or (not local_loss, loss.py:111-113)
    the global rows against themselves."""
    img, txt, t_img, t_txt = inputs
    b = img.shape[0] // ws
    if local_loss or ws == 1:
        sl = slice(r * b, (r + 1) * b)
        return (img[sl], txt[sl], img, txt, t_img[sl], t_txt[sl], t_img, t_txt), r * b
    return (img, txt, img, txt, t_img, t_txt, t_img, t_txt), 0


def route(per, r: int, b: int, ws: int, local_loss: bool, gather_with_grad: bool):
    """(d image_features, d text_features) of rank r from every rank's (d_x_img, d_x_txt, d_y_img, d_y_txt, ...), the gathered side
    routed as gather_features routes it: nothing flows back through a detached gather except the own chunk put back when not
    ``local_loss``; with ``gather_with_grad`` every rank's gathered-side gradient is summed and each rank keeps its own rows."""
    sl = slice(r * b, (r + 1) * b)
    d_xi, d_xt, d_yi, d_yt = per[r][:4]
    if ws == 1:
        return d_xi + d_yi, d_xt + d_yt
    if local_loss:
        if gather_with_grad:
            return d_xi + sum(p[2] for p in per)[sl], d_xt + sum(p[3] for p in per)[sl]
        return d_xi, d_xt
    if gather_with_grad:
        return sum(p[0] + p[2] for p in per)[sl], sum(p[1] + p[3] for p in per)[sl]
    return (d_xi + d_yi)[sl], (d_xt + d_yt)[sl]


def per_rank(inputs, s, st, ws: int, local_loss: bool, gather_with_grad: bool, g_c: float = 1.0, g_d: float = 1.0):
    """Per rank (contrastive, distill, d image_features [b, E], d text_features [b, E], d s) at world size ``ws``."""
    b = inputs[0].shape[0] // ws
    per, losses = [], []
    for r in range(ws):
        args, off = rank_args(inputs, r, ws, local_loss)
        per.append(strip_grads(*args, s, st, off, g_c, g_d))
        losses.append(strip_losses(*args, s, st, off))
    return [(losses[r][0], losses[r][1]) + route(per, r, b, ws, local_loss, gather_with_grad) + (per[r][4],) for r in range(ws)]
