"""The arithmetic of the gradient-ascent loop (openvision_amd/csrc/ascent.hip, openvision_amd/gradient_ascent.py) restated in torch.

Every function computes in the dtype of its inputs.  Called on fp32 tensors it performs the kernels' operations in the kernels'
order, one IEEE rounding per operation (the fp32 form); called on fp64 tensors it is the reference the bounds are measured against
(the fp64 form).  Sums whose order the kernels fix differently (lanes, waves, slabs) are plain torch sums here: the tests bound them
by their length.  A plain helper, not a test module."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24            # fp32 unit roundoff
U64 = 2.0 ** -53


def gamma(n, u=U):
    return n * u / (1 - n * u)


# ---- the image side ----------------------------------------------------------------------------------------------------------------------
def affine(img, mats, mean, std):
    """ov_ga_affine: img [3,S,S], mats [B,6] (inverse pixel maps), mean / std [3] -> [B,3,S,S].  Four taps around (sx, sy), zero outside
    the image, weights as grid_sample forms them, summed in tap order; then (v - mean) / std."""
    s = img.shape[-1]
    dt = img.dtype
    ar = torch.arange(s, dtype=dt)
    y, x = torch.meshgrid(ar, ar, indexing="ij")
    m = mats.to(dt)
    a = [m[:, i].view(-1, 1, 1) for i in range(6)]
    sx = (a[0] * x + a[1] * y) + a[2]
    sy = (a[3] * x + a[4] * y) + a[5]
    x0, y0 = sx.floor(), sy.floor()
    wx1, wy1 = sx - x0, sy - y0
    wx0, wy0 = (x0 + 1) - sx, (y0 + 1) - sy

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < s) & (xx >= 0) & (xx < s)
        yi, xi = yy.clamp(0, s - 1).long(), xx.clamp(0, s - 1).long()
        return torch.where(ok.unsqueeze(1), img[:, yi, xi].permute(1, 0, 2, 3), torch.zeros((), dtype=dt))

    w = [(wx0 * wy0).unsqueeze(1), (wx1 * wy0).unsqueeze(1), (wx0 * wy1).unsqueeze(1), (wx1 * wy1).unsqueeze(1)]
    v = ((tap(y0, x0) * w[0] + tap(y0, x0 + 1) * w[1]) + tap(y0 + 1, x0) * w[2]) + tap(y0 + 1, x0 + 1) * w[3]
    return (v - mean.to(dt).view(1, 3, 1, 1)) / std.to(dt).view(1, 3, 1, 1)


def affine_grid_sample(img, mats, mean, std):
    """The same through F.affine_grid + F.grid_sample('bilinear', 'zeros', align_corners=False) on affine_theta's theta."""
    from openvision_amd.gradient_ascent import affine_theta
    s = img.shape[-1]
    b = mats.shape[0]
    theta = affine_theta(mats.to(img.dtype), s, s)
    grid = F.affine_grid(theta, (b, 3, s, s), align_corners=False)
    v = F.grid_sample(img.unsqueeze(0).expand(b, -1, -1, -1), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return (v - mean.to(img.dtype).view(1, 3, 1, 1)) / std.to(img.dtype).view(1, 3, 1, 1)


def affine_source(mats, s, dtype=torch.float64):
    """(sx, sy) [B,S,S] of every destination pixel, and sum |a0 x| + |a1 y| + |a2| etc.: what the bound of the rotations is made of."""
    ar = torch.arange(s, dtype=dtype)
    y, x = torch.meshgrid(ar, ar, indexing="ij")
    m = mats.to(dtype)
    a = [m[:, i].view(-1, 1, 1) for i in range(6)]
    mag_x = (a[0] * x).abs() + (a[1] * y).abs() + a[2].abs()
    mag_y = (a[3] * x).abs() + (a[4] * y).abs() + a[5].abs()
    return a[0] * x + a[1] * y + a[2], a[3] * x + a[4] * y + a[5], mag_x, mag_y


# ---- the tokens ------------------------------------------------------------------------------------------------------------------------
def gumbel_z(normu, e, tau):
    """z = (normu - log e) / tau.  The logarithm is taken in double and rounded once to the dtype: in fp32 the correctly rounded
    logarithm, which is what the kernels take (a float library logarithm differs from one library to the next in the last bit)."""
    return (normu - e.double().log().to(normu.dtype)) / torch.tensor(tau, dtype=normu.dtype)


def sample(z):
    """(idx: first argmax, zmax, zsum = sum exp(z - zmax), ys = exp(z - zmax) / zsum) over the last dimension."""
    zmax, idx = z.max(dim=-1)
    ex = (z - zmax.unsqueeze(-1)).exp()
    zsum = ex.sum(dim=-1)
    return idx, zmax, zsum, ex / zsum.unsqueeze(-1)


def token_grad(dx, w, ys, tau):
    """gy = dX W^T, c = sum_v gy ys, g = ys (gy - c) / tau: d loss / d normu for upstream dX at the tower's input rows."""
    gy = dx @ w.t()
    c = (gy * ys).sum(dim=-1, keepdim=True)
    return gy, c, (ys * (gy - c)) / torch.tensor(tau, dtype=ys.dtype)


def adam_constants(t, lr, betas, eps, dtype):
    """The scalars of step t as the kernel holds them.  fp32: rounded to float after the host's double arithmetic."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    vals = dict(w=1.0 - b1, b2=b2, w2=1.0 - b2, bc2_sqrt=math.sqrt(bc2), eps=eps, step=lr / bc1)
    return {k: torch.tensor(v, dtype=dtype) for k, v in vals.items()}


def adam_step(p, g, ea, es, k):
    """torch.optim.Adam's single-tensor update in its operation order on constants ``k`` (adam_constants); returns (p, ea, es)."""
    d = g - ea
    ea = ea + k["w"] * d if float(k["w"]) < 0.5 else g - d * (1 - k["w"])
    es = es * k["b2"] + (k["w2"] * g) * g
    denom = es.sqrt() / k["bc2_sqrt"] + k["eps"]
    return p - k["step"] * (ea / denom), ea, es


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
def cosine_loss(tx, img, eps=1e-8):
    """loss1[j] = -100 mean_i cos(tx_j, img_i) and d mean_j loss1[j] / d tx, by the explicit formula of the kernel."""
    b = tx.shape[0]
    nt, ni = tx.norm(dim=-1), img.norm(dim=-1)
    mt, mi = nt.clamp_min(eps), ni.clamp_min(eps)
    dots = tx @ img.t()
    cos = dots / (mt.unsqueeze(1) * mi.unsqueeze(0))
    loss1 = -100.0 * (cos.sum(dim=1) / b)
    live = (nt > eps).to(tx.dtype)
    first = (img.unsqueeze(0) / (mt.view(b, 1, 1) * mi.view(1, b, 1))).sum(dim=1)
    second = ((dots / ((mt * mt).unsqueeze(1) * mi.unsqueeze(0) * nt.clamp_min(1e-300 if tx.dtype == torch.float64 else 1e-37).unsqueeze(1)))
              .sum(dim=1, keepdim=True) * tx) * live.unsqueeze(1)
    return loss1, (-100.0 / (b * b)) * (first - second)


def cosine_loss_eager(tx, img):
    """The script's line 246 on torch.cosine_similarity."""
    b = tx.shape[0]
    return -100 * torch.cosine_similarity(tx.unsqueeze(0), img.unsqueeze(1), -1).view(-1, b).T.mean(1)
