"""Host-side float64 torch restatement of the contrastive term OpenVision trains with: ``bidirectional_contrastive_loss(zimg, ztxt_1,
ztxt_2, t, local_loss=True)`` (reference src/losses/common.py:120-189), generalised from two caption sets to C.  jax is not installed
anywhere this project runs, so parity with the JAX function is BY RESTATEMENT: ``strip_loss`` follows common.py:139-171 line by line.
What pins it numerically is the reference's own torch ``open_clip.loss.ClipLoss`` evaluated once per caption set and averaged
(tests/golden/multicap_grad.npz, made by tests/golden/make_golden_multicap.py); tests/test_multicap_cpu.py checks the restatement
against that fixture before any kernel runs.

Also: the fixture's cases and their inputs, regenerated from recorded seeds (the fixture stores checksums, not the inputs)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

# name, world_size, b (rows per rank), E, C (caption sets), local_loss, gather_with_grad, s (the multiplier), seed.
# s is chosen per width so that the loss is of order 0.5: well below log N (the sets are matched to the images), yet large enough
# that the fp32 kernels' 1e-5 RELATIVE bound on the loss is a statement about lse - diag and not about its cancellation (with
# s = 100 these inputs give losses of 1e-20).  normalize(img / 2 + noise / 20) sits at cosine ~0.78 to its image at E = 64 and
# ~0.34 at E = 768.
CASES = [
    ("ws1_b13_e64_c2", 1, 13, 64, 2, True, False, 5.0, 201),
    ("ws1_b16_e64_c1", 1, 16, 64, 1, True, False, 5.0, 202),
    ("ws2_b13_e64_c2_local", 2, 13, 64, 2, True, False, 5.0, 203),
    ("ws2_b16_e64_c3_local_gwg", 2, 16, 64, 3, True, True, 5.0, 204),
    ("ws3_b13_e64_c2_global", 3, 13, 64, 2, False, False, 5.0, 205),
    ("ws3_b16_e64_c3_local", 3, 16, 64, 3, True, False, 5.0, 206),
    ("ws3_b13_e64_c1_local_gwg", 3, 13, 64, 1, True, True, 5.0, 207),
    ("ws2_b16_e64_c2_global", 2, 16, 64, 2, False, False, 5.0, 208),
    ("ws2_b13_e768_c2_local_gwg", 2, 13, 768, 2, True, True, 10.0, 209),
]


def make_inputs(n: int, e: int, c: int, seed: int, dtype=torch.float64):
    """[n, E] image embeddings and [C, n, E] caption-set embeddings, L2-normalised in fp32 and returned as ``dtype`` holding fp32
    values.  Every set is its image at half weight plus its OWN noise draw: the sets are correlated with the images and differ
    from each other."""
    g = torch.Generator().manual_seed(seed)
    img = F.normalize(torch.randn(n, e, generator=g), dim=-1)
    sets = torch.stack([F.normalize(img * 0.5 + torch.randn(n, e, generator=g) * 0.05, dim=-1) for _ in range(c)])
    return img.to(dtype), sets.to(dtype)


def case_inputs(ws: int, b: int, e: int, c: int, seed: int):
    """The global sets of a case: rank r owns rows [r b, (r + 1) b) of the images and of every caption set."""
    return make_inputs(ws * b, e, c, seed)


def stack_local(sets: torch.Tensor, rank: int, b: int) -> torch.Tensor:
    """[C, N, E] -> this rank's stacked [C b, E] text rows (set c in rows c b ...: the reference's concatenated captions)."""
    return torch.cat([sets[c, rank * b:(rank + 1) * b] for c in range(sets.shape[0])], dim=0)


def strip_loss(img, txt_stacked, all_img, all_txt_sets, s, rank: int, C: int):
    """common.py:139-171 with C sets instead of two.  img [b, E], txt_stacked [C b, E], all_img [N, E], all_txt_sets [C, N, E]."""
    b = img.shape[0]
    idx = torch.arange(b)
    local_losses = []
    for c in range(C):
        local_txt = txt_stacked[c * b:(c + 1) * b]                                   # ztxt[:half] / ztxt[half:]
        ztxt = all_txt_sets[c]
        logits_img = torch.log_softmax(img @ ztxt.T * s, dim=1)                      # :140-141 / :146-147
        logits_txt = torch.log_softmax(local_txt @ all_img.T * s, dim=1)             # :142-143 / :148-149
        l1 = -logits_img[idx, idx + rank * b]                                        # :155-156 / :161-162
        l2 = -logits_txt[idx, idx + rank * b]                                        # :157-158 / :163-164
        local_losses.append(0.5 * (l1 + l2))                                         # :167-168
    return (sum(local_losses) / C).mean()                                            # :171 (pmean is left to the gradient averaging)


def strip_terms(img, txt_stacked, all_img, all_txt_sets, s, rank: int, C: int):
    """[4 C, b]: per set the rows lse_img, diag_img, lse_txt, diag_txt (what ov_clip_loss_multi writes as ``terms``)."""
    b = img.shape[0]
    idx = torch.arange(b)
    rows = []
    for c in range(C):
        a = img @ all_txt_sets[c].T * s
        t = txt_stacked[c * b:(c + 1) * b] @ all_img.T * s
        rows += [torch.logsumexp(a, 1), a[idx, idx + rank * b], torch.logsumexp(t, 1), t[idx, idx + rank * b]]
    return torch.stack(rows)


def strip_grads(img, txt_stacked, all_img, all_txt_sets, s, rank: int, C: int, grad: float = 1.0):
    """Closed form of ``strip_loss``'s gradient, every argument an independent leaf.  With P = (softmax - onehot) * grad / (2 C b)
    per strip:  d img = s sum_c P_img,c all_txt_c,  d txt_c = s P_txt,c all_img,  d all_img = s sum_c P_txt,c^T txt_c,
    d all_txt_c = s P_img,c^T img,  d s = sum over every strip of P .* dots.
    Returns (d_img [b, E], d_txt [C b, E], d_all_img [N, E], d_all_txt [C, N, E], d_s)."""
    b = img.shape[0]
    idx = torch.arange(b)
    d_img, d_all_img, d_s = torch.zeros_like(img), torch.zeros_like(all_img), 0.0
    d_txt, d_all_txt = [], []
    for c in range(C):
        txt = txt_stacked[c * b:(c + 1) * b]
        di, dt = img @ all_txt_sets[c].T, txt @ all_img.T
        pi, pt = torch.softmax(s * di, 1), torch.softmax(s * dt, 1)
        pi[idx, idx + rank * b] -= 1.0
        pt[idx, idx + rank * b] -= 1.0
        pi, pt = pi * (grad / (2 * C * b)), pt * (grad / (2 * C * b))
        d_img = d_img + s * pi @ all_txt_sets[c]
        d_all_img = d_all_img + s * pt.T @ txt
        d_txt.append(s * pt @ all_img)
        d_all_txt.append(s * pi.T @ img)
        d_s = d_s + (pi * di).sum() + (pt * dt).sum()
    return d_img, torch.cat(d_txt, dim=0), d_all_img, torch.stack(d_all_txt), d_s


def per_rank(img_all, sets_all, s, ws: int, local_loss: bool, gather_with_grad: bool):
    """Per rank (loss, d image_features [b, E], d text_features [C b, E], d s) at world size ``ws``, the gathered side routed as
    gather_features routes it (open_clip/loss.py:19-63): nothing flows back through a detached gather except the own chunk put
    back when not ``local_loss``; with ``gather_with_grad`` every rank's gathered-side gradient is summed and each rank keeps its
    own rows."""
    c, n = sets_all.shape[0], img_all.shape[0]
    b = n // ws
    glob = torch.cat(list(sets_all), dim=0)                                          # the stacked global text set [C N, E]
    per, losses = [], []
    for r in range(ws):
        if local_loss or ws == 1:
            args = (img_all[r * b:(r + 1) * b], stack_local(sets_all, r, b), img_all, sets_all, s, r, c)
        else:
            args = (img_all, glob, img_all, sets_all, s, 0, c)
        per.append(strip_grads(*args))
        losses.append(strip_loss(*args))
    out = []
    for r in range(ws):
        sl = slice(r * b, (r + 1) * b)
        d_img, d_txt, d_ai, d_at, d_s = per[r]
        if ws == 1:
            gi, gt = d_img + d_ai, d_txt + torch.cat(list(d_at), dim=0)
        elif local_loss:
            gi, gt = d_img.clone(), d_txt.clone()
            if gather_with_grad:
                gi = gi + sum(p[2] for p in per)[sl]
                gt = gt + stack_local(sum(p[3] for p in per), r, b)
        else:
            tot_i = [p[0] + p[2] for p in per]                                       # local rows ARE the global rows here
            tot_t = [p[1].view(c, n, -1) + p[3] for p in per]
            if gather_with_grad:
                gi, gt = sum(tot_i)[sl], stack_local(sum(tot_t), r, b)
            else:
                gi, gt = tot_i[r][sl], stack_local(tot_t[r], r, b)
        out.append((losses[r], gi, gt, d_s))
    return out
