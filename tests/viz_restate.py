"""The arithmetic of the feature-visualisation loop (ov-feature-visualization.py:90-139, 203-221 with cliptoolsoptimized.py's RepeatBatch,
ColorJitter, GaussianNoise, Tile, Jitter, Clip, TotalVariation), restated in torch for the tests of openvision_amd.visualize's loop and of
csrc/vizloop.hip.  A plain helper, not a conftest.  Works in the dtype of its inputs: fp32 restates what the script computes, fp64 is the
reference the kernels' bounds are taken against."""
import math
import random

import torch

U = 2.0 ** -24          # fp32 unit round-off


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
class _ColorJitter:
    """Shuffles at construction and again in every forward (shuffle_every=True): two rand per shuffle."""

    def __init__(self, batch, mean_p, std_p):
        self.batch, self.mean_p, self.std_p = batch, mean_p, std_p
        self.shuffle()

    def shuffle(self):
        self.mean = (torch.rand((self.batch, 3, 1, 1)) - 0.5) * 2 * self.mean_p
        self.std = ((torch.rand((self.batch, 3, 1, 1)) - 0.5) * 2 * self.std_p).exp()


class _GaussianNoise:
    """Shuffles at construction and in every forward: one randn per shuffle, scaled by a counter that runs down and wraps."""

    def __init__(self, batch, std_p, max_iter):
        self.batch, self.std_p, self.max_iter = batch, std_p, max_iter
        self.rem = max_iter - 1
        self.shuffle()

    def shuffle(self):
        self.std = torch.randn(self.batch, 3, 1, 1) * self.rem * self.std_p / self.max_iter
        self.rem = (self.rem - 1 + self.max_iter) % self.max_iter


def script_draws(steps, n, repeat, size, mean_p=1.0, std_p=1.0, noise_p=0.5, max_iter=400, lim=32):
    """The script's random sequence for one (layer, feature): the two constructors, new_init's image, then per iteration the two
    shuffles and Jitter's two randint.  Returns (image [n,3,size,size], means, stds, noises (lists of [B,3,1,1]), offsets)."""
    batch = repeat * n
    cj, gn = _ColorJitter(batch, mean_p, std_p), _GaussianNoise(batch, noise_p, max_iter)
    image = torch.rand(size=(n, 3, size, size))
    means, stds, noises, offsets = [], [], [], []
    for _ in range(steps + 1):
        cj.shuffle()
        gn.shuffle()
        means.append(cj.mean)
        stds.append(cj.std)
        noises.append(gn.std)
        offsets.append((random.randint(-lim, lim), random.randint(-lim, lim)))
    return image, means, stds, noises, offsets


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
def augment(img, mean, std, noise, off1, off2, repeat):
    """RepeatBatch -> ColorJitter -> GaussianNoise -> Tile(1) -> Jitter; mean / std / noise [B,3,1,1]."""
    x = img.repeat(repeat, 1, 1, 1)
    x = (x - mean) / std
    x = x + noise
    return torch.roll(x, shifts=(off1, off2), dims=(2, 3))


def patch_rows(x, p):
    """[B,3,S,S] -> [B*g*g, 3*p*p]: conv1's operand rows (stride = kernel = p), column c*p*p + i*p + j."""
    b, _, s, _ = x.shape
    g = s // p
    return x.reshape(b, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(b * g * g, 3 * p * p)


def unpatch_rows(rows, b, s, p):
    """patch_rows' inverse on the first 3*p*p columns."""
    g = s // p
    return rows[:, :3 * p * p].reshape(b, g, g, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(b, 3, s, s)


# ---- total variation -------------------------------------------------------------------------------------------------------------------
def tv_fields(x):
    return [x[:, :, :, 1:] - x[:, :, :, :-1], x[:, :, 1:, :] - x[:, :, :-1, :], x[:, :, 1:, 1:] - x[:, :, :-1, :-1],
            x[:, :, 1:, :-1] - x[:, :, :-1, 1:]]


def tv_norms(x):
    """[4, B, 3]: the L2 norm of each difference field over each plane."""
    return torch.stack([f.norm(p=2, dim=(2, 3)) for f in tv_fields(x)])


def tv_value(x, size):
    return sum(f.norm(p=2, dim=(2, 3)).mean() for f in tv_fields(x)) * (x.shape[-2] * x.shape[-1]) / (size * size)


_ENDS = [((slice(None), slice(1, None)), (slice(None), slice(None, -1))),          # field -> (its + end, its - end) as (rows, columns)
         ((slice(1, None), slice(None)), (slice(None, -1), slice(None))),
         ((slice(1, None), slice(1, None)), (slice(None, -1), slice(None, -1))),
         ((slice(1, None), slice(None, -1)), (slice(None, -1), slice(1, None)))]


def tv_grad_terms(x, size):
    """[8, B, 3, S, S]: the up to eight terms +-diff / (norm * 3B) * S^2 / size^2 of d tv / d x at each pixel (0 where the pixel is not
    an end of that difference, and for a plane whose norm is 0)."""
    b, _, s, _ = x.shape
    out = x.new_zeros(8, b, 3, s, s)
    scale = (s * s) / (size * size) / (3 * b)
    for k, (f, (plus, minus)) in enumerate(zip(tv_fields(x), _ENDS)):
        nrm = f.norm(p=2, dim=(2, 3), keepdim=True)
        t = torch.where(nrm > 0, f / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(f)) * scale
        out[2 * k][:, :, plus[0], plus[1]] = t
        out[2 * k + 1][:, :, minus[0], minus[1]] = -t
    return out


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def closed_form_grad(g_aug, aug, std, off1, off2, repeat, c_tv, size):
    """d loss / d img for loss = <objective part> + c_tv * tv(aug): g_aug = d objective / d aug [B,3,S,S]."""
    d_aug = g_aug + c_tv * tv_grad_terms(aug, size).sum(dim=0)
    d = torch.roll(d_aug, shifts=(-off1, -off2), dims=(2, 3)) / std
    return d.view(repeat, -1, *d.shape[1:]).sum(dim=0)


def grad_bound(g_aug, aug, std, off1, off2, repeat, c_tv, size):
    """u * sum_r ((R + 2) |G_r| + (R + n + 6) sum_k |t_rk|) / std_r per pixel of img, n = the differences of a diagonal field (the
    smallest of the four counts); everything in fp64."""
    s = aug.shape[-1]
    n = (s - 1) * (s - 1)
    t = (c_tv * tv_grad_terms(aug, size)).abs().sum(dim=0)
    per_row = ((repeat + 2) * g_aug.abs() + (repeat + n + 6) * t) / std
    per_row = torch.roll(per_row, shifts=(-off1, -off2), dims=(2, 3))
    return U * per_row.view(repeat, -1, *per_row.shape[1:]).sum(dim=0)


# ---- update ----------------------------------------------------------------------------------------------------------------------------
def cosine_lr(steps, lr):
    return [lr * (1.0 + math.cos(math.pi * i / steps)) / 2.0 for i in range(steps + 1)]


def adamax_clip(img, g, ea, ei, lr_i, t, b1=0.5, b2=0.99, eps=1e-8, lo=0.0, hi=1.0):
    """Iteration t (1-based) of Adamax at learning rate lr_i, then the clamp: (img, ea, ei) afterwards."""
    ea = ea + (g - ea) * (1 - b1)
    ei = torch.maximum(ei * b2, g.abs() + eps)
    clr = lr_i / (1 - b1 ** t)
    return (img - clr * ea / ei).clamp(lo, hi), ea, ei
