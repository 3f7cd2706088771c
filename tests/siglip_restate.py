"""Host-side torch restatement of the SigLIP loss (reference open_clip/loss.py:307-414) in the transport this project uses: one
all-gather of the text features, the whole [b, N] strip per rank, and the gathered side's gradient summed over ranks (own chunk
kept).  The reference passes text blocks round a neighbour-exchange ring instead; tests/golden/siglip_grad.npz holds what its
autograd gives per rank, and tests/test_siglip_cpu.py pins this restatement to it before any kernel runs.

Also: the fixture's cases and their inputs, regenerated from recorded seeds (the fixture stores checksums, not the inputs)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

# name, world_size, b (rows per rank), E, s (the multiplier), beta, bidir, seed
CASES = [
    ("ws1_b13_e40_init", 1, 13, 40, 10.0, -10.0, True, 101),
    ("ws2_b13_e40_init_bidir", 2, 13, 40, 10.0, -10.0, True, 102),
    ("ws2_b13_e40_trained_uni", 2, 13, 40, 100.0, -15.0, False, 103),
    ("ws3_b13_e40_trained_bidir", 3, 13, 40, 100.0, -15.0, True, 104),
    ("ws3_b13_e40_init_uni", 3, 13, 40, 10.0, -10.0, False, 105),
    ("ws4_b64_e40_init_bidir", 4, 64, 40, 10.0, -10.0, True, 106),
    ("ws4_b13_e40_trained_uni", 4, 13, 40, 100.0, -15.0, False, 107),
    ("ws4_b13_e40_trained_bidir", 4, 13, 40, 100.0, -15.0, True, 108),
    ("ws2_b24_e768_trained_bidir", 2, 24, 768, 100.0, -15.0, True, 109),
]


def case_inputs(ws: int, b: int, e: int, seed: int):
    """[N, E] image and text embeddings (N = ws * b, rank r owns rows [r b, (r + 1) b)), L2-normalised in fp32 and returned as
    float64 holding fp32 values.  Text i is image i plus noise: matched pairs sit at cosine ~0.8-0.95, so with s ~ 100 and
    beta = -15 their logits are strongly positive while the negatives spread round -15."""
    g = torch.Generator().manual_seed(seed)
    n = ws * b
    img = F.normalize(torch.randn(n, e, generator=g), dim=-1)
    txt = F.normalize(img + torch.randn(n, e, generator=g) * 0.6 / e ** 0.5 * torch.rand(n, 1, generator=g) * 2, dim=-1)
    return img.double(), txt.double()


def strip_loss(img, all_txt, scale, bias, rank: int):
    """The loss of rank ``rank``: (1/b) sum softplus(-l z) over its [b, N] strip, z = s x.y + beta, l = +1 at j = i + b rank.
    Differentiable torch; what the reference's ring sums block by block (loss.py:349-358)."""
    b = img.shape[0]
    z = scale * img @ all_txt.T
    if bias is not None:
        z = z + bias
    lab = -torch.ones_like(z)
    lab[torch.arange(b), torch.arange(b) + b * rank] = 1.0
    return -F.logsigmoid(lab * z).sum() / b


def strip_grads(img, all_txt, scale, bias, rank: int, grad: float = 1.0):
    """Closed form of the strip's gradient, every argument an independent leaf: g = -l sigmoid(-l z) / b * grad, then
    d img = s g all_txt, d all_txt = s g^T img, d s = sum g (img all_txt^T), d beta = sum g.  Returns (d_img, d_all_txt, d_s, d_beta)."""
    b = img.shape[0]
    dots = img @ all_txt.T
    z = scale * dots + (bias if bias is not None else 0.0)
    lab = -torch.ones_like(z)
    lab[torch.arange(b), torch.arange(b) + b * rank] = 1.0
    g = -lab * torch.sigmoid(-lab * z) / b * grad
    return scale * g @ all_txt, scale * g.T @ img, (g * dots).sum(), g.sum()


def per_rank(img_all, txt_all, scale, bias, ws: int):
    """Per rank: (loss, d image_features, d text_features, d s, d beta) at world_size ``ws`` in the all-gather transport:
    d text_features of rank r = rows [r b, (r + 1) b) of the gathered-side gradient summed over all ranks."""
    n = img_all.shape[0]
    b = n // ws
    parts = [strip_grads(img_all[r * b:(r + 1) * b], txt_all, scale, bias, r) for r in range(ws)]
    d_all = sum(p[1] for p in parts)
    out = []
    for r in range(ws):
        loss = strip_loss(img_all[r * b:(r + 1) * b], txt_all, scale, bias, r)
        out.append((loss, parts[r][0], d_all[r * b:(r + 1) * b], parts[r][2], parts[r][3]))
    return out
