"""Host-side float64 closed form of the InfoNCE gradient of one WINDOW of a fixed bank (gradient accumulation,
``ov_clip_loss_window_backward``): with all N rows and the two log-sum-exp vectors of the whole bank held fixed, the gradient of
    1 / (2 C norm_rows) sum_c sum_{i < N} [ lse(A_c[i, :]) - A_c[i, i] + lse(B_c[i, :]) - B_c[i, i] ],   A_c = s img txt_c^T = B_c^T
with respect to the rows [w0, w0 + b).  A window row is a row of its own strip (softmax under its own lse) and a column of every
other row's strip (softmax under that row's lse), and its label is subtracted once on each account:
    d img_i   = s / (2 C n) sum_c sum_k [ exp(A_c[i,k] - lse_img,c[i]) + exp(A_c[i,k] - lse_txt,c[k]) - 2 [k = i] ] txt_c,k
    d txt_c,j = s / (2 C n)       sum_k [ exp(B_c[j,k] - lse_txt,c[j]) + exp(B_c[j,k] - lse_img,c[k]) - 2 [k = j] ] img_k
The ``d s`` share is taken from the image-side strips alone and the loss share from the window's rows of ``terms``, so disjoint
windows that cover the bank sum to the full gradient and the full loss.  ``terms`` is ``multicap_restate.strip_terms`` of the bank."""
from __future__ import annotations

import torch

import multicap_restate as MR


def bank_terms(img_all: torch.Tensor, sets_all: torch.Tensor, s: float) -> torch.Tensor:
    """[4 C, N]: what ov_clip_loss_multi writes for b = N, label_offset = 0 over the bank img_all [N, E], sets_all [C, N, E]."""
    return MR.strip_terms(img_all, torch.cat(list(sets_all), dim=0), img_all, sets_all, s, 0, sets_all.shape[0])


def window(img_all: torch.Tensor, sets_all: torch.Tensor, s: float, w0: int, b: int, norm_rows: int, terms: torch.Tensor = None,
           grad: float = 1.0):
    """(d_img [b, E], d_txt [C b, E] stacked set by set, the d_s share, the loss share) of window [w0, w0 + b)."""
    c, n = sets_all.shape[0], img_all.shape[0]
    assert 0 <= w0 and b > 0 and w0 + b <= n and norm_rows > 0
    terms = bank_terms(img_all, sets_all, s) if terms is None else terms
    sl, idx = slice(w0, w0 + b), torch.arange(b)
    coef = grad / (2.0 * c * norm_rows)
    d_img, d_txt, d_s, loss = torch.zeros_like(img_all[sl]), [], 0.0, 0.0
    for k in range(c):
        lse_i, diag_i, lse_t, diag_t = terms[4 * k:4 * k + 4]
        dots = img_all[sl] @ sets_all[k].T                                            # image side: [b, N]
        p = torch.exp(s * dots - lse_i[sl, None]) + torch.exp(s * dots - lse_t[None, :])
        p[idx, w0 + idx] -= 2.0
        d_img = d_img + coef * s * p @ sets_all[k]
        d_s = d_s + coef * (p * dots).sum()
        dots = sets_all[k][sl] @ img_all.T                                            # text side of set k: [b, N]
        q = torch.exp(s * dots - lse_t[sl, None]) + torch.exp(s * dots - lse_i[None, :])
        q[idx, w0 + idx] -= 2.0
        d_txt.append(coef * s * q @ img_all)
        loss = loss + coef * ((lse_i - diag_i) + (lse_t - diag_t))[sl].sum()
    return d_img, torch.cat(d_txt, dim=0), d_s, loss


def stack_window(sets_all: torch.Tensor, w0: int, b: int) -> torch.Tensor:
    """[C, N, E] -> the window's stacked [C b, E] text rows."""
    return torch.cat([sets_all[k, w0:w0 + b] for k in range(sets_all.shape[0])], dim=0)
