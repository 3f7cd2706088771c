"""Feature visualisation: the differentiable MLP-feature objective of ``ov-feature-visualization.py`` on the HIP path.

The reference script reads one hidden unit of one vision block's MLP through a forward hook on ``resblocks[layer].mlp.gelu``
(``ViTEnsFeatHook(ClipOVGeLUHook(model, sl=slice(layer, layer + 1)), key='high', feat=feature)``: ov-feature-visualization.py:211,
cliptoolsoptimized.py:990-999, 1149-1164) and back-propagates to the pixels.  Here GELU is fused into the c_fc epilogue, so the unit is
computed directly:

    x_l   = blocks[0 .. layer)(embed(image))                       ov_tower_forward_saving / ov_tower_backward_input
    x1    = x_l + out_proj(attn(ln_1(x_l)))                        ov_block_attn_forward_saving / ov_block_attn_backward_input
    m_b   = mean_{t >= 1} gelu(ln_2(x1) . W_fc[f] + b_fc[f])       ov_mlp_feature_forward / ov_mlp_feature_backward
    loss  = -(1 / B^2) sum_b m_b                                   (the reference's ``-all_feats[:B, f].diag().mean()``)

Blocks after ``layer`` do not change the value and are not run; nothing of the tap block's MLP but the one column is computed.  The
model's parameters are constants: the backward computes input gradients only and writes no ``.grad``.  The path is bf16 whatever
``set_precision`` says.  In the script, line 211 becomes ``loss += MLPFeatureLoss(premodel, layer, feature)``.

``FeatureVisualizer`` is the script's whole loop around that objective (``ImageNetVisualizer``, ov-feature-visualization.py:90-139, with
the augmentations, losses and optimiser of :203-221) as HIP launches: per step

    ov_viz_augment                 RepeatBatch -> ColorJitter -> GaussianNoise -> Tile(1) -> Jitter, written as conv1 operand rows
    training._patch_tokens_forward, ov_convert         ov_gemm, ov_patch_keep_assemble (mlp_feature's arithmetic); the bf16 tokens
    _feature_forward / _feature_backward               the objective's own launches, as under ``mlp_feature``
    ov_viz_tv                      TotalVariation's plane norms
    ov_convert, training._patch_tokens_backward        ov_patch_keep_assemble_backward, ov_linear_backward: the patch rows' dcols only
    ov_viz_augment_backward        d loss / d img and the step's (loss, feature term, tv term) row of ``history``
    ov_adamax_clip_step            torch.optim.Adamax + CosineAnnealingLR + Clip

Every random draw of the run is made on the host up front (``draw_tables``), in the script's order, and uploaded once: a step makes no
host-to-device copy, no ``.item()`` and no eager torch arithmetic.
"""
from __future__ import annotations

import ctypes as C
import math
import random

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .model import _pack_matrix, _round_up
from .training import _patch_tokens_backward, _patch_tokens_eager, _patch_tokens_forward, _pool

__all__ = ["mlp_feature", "MLPFeatureLoss", "FeatureVisualizer", "draw_tables", "new_init", "fix_random_seed"]


def _a256(n: int) -> int:
    return (n + 255) // 256 * 256


class _FeatureState:
    """What _feature_forward keeps for _feature_backward: the forward's handle, weights, pooled buffers and the tap buffer's sections."""
    __slots__ = ("pool", "tower", "tap_weights", "cfg1", "meta", "xb", "tap", "sections", "saved", "gens")


def _feature_forward(visual, layer, feature, xb, keep_state):
    """Blocks [0, layer), the tap block's attention half and the tap kernels on xb (bf16 [B, L, D], contiguous; OVERWRITTEN with the tap
    block's input): (m fp32 [B], the state of _feature_backward or None when keep_state is false)."""
    lib = _lib.load()
    tr = visual.transformer
    blocks = list(tr.resblocks)[:layer + 1]
    b0 = blocks[0]
    d, heads, mlp, mlp_pad = b0.attn.embed_dim, b0.attn.num_heads, b0.mlp_dim, b0.mlp_pad
    eps, tanh = float(b0.ln_2.eps), int(b0.gelu_tanh)
    bsz, seq, _ = xb.shape
    m = bsz * seq
    pool = _pool(tr)
    saved = tower = None
    if layer > 0:                                   # blocks [0, layer): xb becomes the tap block's input
        tower = tr._cache.get(blocks[:layer], plain=True)
        saved = pool.take(lib.ov_tower_saved_bytes(tower.handle, bsz, seq), xb.device, "saved")
        nbytes = lib.ov_tower_workspace_bytes(tower.handle, bsz, seq)
        ws = pool.take(nbytes, xb.device)
        check(lib.ov_tower_forward_saving(tower.handle, ptr(xb), ptr(saved), bsz, seq, ptr(ws), nbytes, stream_ptr()),
              "ov_tower_forward_saving")
        pool.give(ws)
    # the tap block: qkv | attention out | x1 | lse | pre, one pooled buffer
    lp = (seq + 31) // 32 * 32
    offs, total = [], 0
    for n in (m * 3 * d * 2, m * d * 2, m * d * 2, bsz * heads * lp * 4, m * 4):
        offs.append(total)
        total += _a256(n)
    tap = pool.take(total, xb.device, "featviz")
    sections = qkv, attn_out, x1, lse, pre = [C.c_void_p(tap.data_ptr() + o) for o in offs]
    cfg1 = _lib.TowerCfg(d, 1, heads, mlp, mlp_pad, tanh, float(b0.ln_1.eps))
    wt, keep = blocks[layer].packed_block(fold_ln=False)          # the tap block's own LayerNorms and weights, ov_block_weights order
    check(lib.ov_block_attn_forward_saving(C.byref(cfg1), C.byref(wt), ptr(xb), qkv, attn_out, x1, lse, bsz, seq, stream_ptr()),
          "ov_block_attn_forward_saving")
    fc_w, fc_b, ln2_w, ln2_b = keep[8], keep[9], keep[6], keep[7]
    mean = torch.empty(bsz, dtype=torch.float32, device=xb.device)
    check(lib.ov_mlp_feature_forward(x1, d, ptr(ln2_w), ptr(ln2_b), ptr(fc_w), d, ptr(fc_b), feature, mlp, tanh, bsz, seq, d, eps, pre,
                                     ptr(mean), stream_ptr()), "ov_mlp_feature_forward")
    if not keep_state:                              # no backward will come: hand the buffers back now
        pool.give(tap)
        if saved is not None:
            pool.give(saved)
        return mean, None
    st = _FeatureState()
    st.pool, st.tower, st.tap_weights, st.cfg1 = pool, tower, (wt, keep), cfg1       # the backward runs the forward's handle and weights
    st.meta = (layer, feature, bsz, seq, d, mlp, tanh, eps)
    st.xb, st.tap, st.sections, st.saved = xb, tap, sections, saved
    st.gens = (tap._ovhip_gen, saved._ovhip_gen if saved is not None else None)
    return mean, st


def _feature_backward(st, dm):
    """d sum_b dm[b] m[b] / d x as bf16 [B * L, D] (dm: device fp32 [B], contiguous); hands the forward's buffers back."""
    lib = _lib.load()
    layer, feature, bsz, seq, d, mlp, tanh, eps = st.meta
    tap, saved, pool = st.tap, st.saved, st.pool
    if tap._ovhip_gen != st.gens[0] or (saved is not None and saved._ovhip_gen != st.gens[1]):
        raise _lib.OvhipError("feature objective: the saved activations of this graph were recycled by a later forward; a second "
                              "backward over the same graph must come before the next forward")
    m = bsz * seq
    qkv, attn_out, x1, lse, pre = st.sections
    wt, keep = st.tap_weights
    handle = st.tower.handle if st.tower is not None else None
    attn_bytes = lib.ov_block_attn_backward_input_workspace_bytes(C.byref(st.cfg1), bsz, seq)
    tower_bytes = lib.ov_tower_backward_input_workspace_bytes(handle, bsz, seq) if handle else 0
    if attn_bytes == 0 or (handle and tower_bytes == 0):
        raise _lib.OvhipError("feature objective: width % 64 == 0 and head_dim % 8 == 0, <= 96 are required")
    dx1_off = _a256(max(attn_bytes, tower_bytes))
    ws = pool.take(dx1_off + m * d * 2, dm.device)
    dx1 = C.c_void_p(ws.data_ptr() + dx1_off)
    dx = torch.empty(m, d, dtype=torch.bfloat16, device=dm.device)
    check(lib.ov_mlp_feature_backward(x1, d, ptr(keep[6]), ptr(keep[8]), d, feature, mlp, tanh, pre, ptr(dm), dx1, d, bsz, seq, d, eps,
                                      stream_ptr()), "ov_mlp_feature_backward")
    check(lib.ov_block_attn_backward_input(C.byref(st.cfg1), C.byref(wt), ptr(st.xb), qkv, attn_out, lse, dx1, ptr(dx), bsz, seq,
                                           ptr(ws), attn_bytes, stream_ptr()), "ov_block_attn_backward_input")
    if handle:
        check(lib.ov_tower_backward_input(handle, ptr(saved), ptr(dx), bsz, seq, ptr(ws), tower_bytes, stream_ptr()),
              "ov_tower_backward_input")
    pool.give(ws)             # ordered on the stream: the next forward's writes come after this backward's reads
    pool.give(tap)
    if saved is not None:
        pool.give(saved)
    return dx


class _FeatureFn(torch.autograd.Function):
    """Blocks [0, layer), the tap block's attention half and the tap kernels as one autograd node: x [B, L, D] -> m [B] (fp32)."""

    @staticmethod
    def forward(ctx, visual, layer, feature, x):
        xb = x.detach().to(torch.bfloat16).contiguous().clone()
        mean, ctx.state = _feature_forward(visual, layer, feature, xb, ctx.needs_input_grad[3])
        ctx.x_dtype = x.dtype
        return mean

    @staticmethod
    def backward(ctx, dmean):
        st = ctx.state
        dx = _feature_backward(st, dmean.detach().float().contiguous())
        return None, None, None, dx.view(st.meta[2], st.meta[3], st.meta[4]).to(ctx.x_dtype)


def _check_args(visual, image, layer: int, feature: int):
    pd = getattr(visual, "patch_dropout", None)
    if visual.training and float(getattr(pd, "prob", 0.0)) > 0:
        raise _lib.OvhipError(f"feature objective: the vision tower is in training mode with patch_dropout = {pd.prob}; the objective reads "
                              "every patch token and does not drop any -- call model.eval() (or visual.eval()) first")
    if not isinstance(visual.ln_pre, torch.nn.Identity):
        raise _lib.OvhipError("feature objective: ln_pre is Identity for OpenVision towers")
    blocks = list(visual.transformer.resblocks)
    if not 0 <= int(layer) < len(blocks):
        raise _lib.OvhipError(f"feature objective: layer {layer} outside [0, {len(blocks)})")
    mlp = blocks[0].mlp_dim
    if not 0 <= int(feature) < mlp:
        raise _lib.OvhipError(f"feature objective: feature {feature} outside [0, {mlp})")
    if not image.is_cuda:
        raise _lib.OvhipError("feature objective: tensors must live on an MI355X device (no CPU fallback)")
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError("image must be [B, 3, H, W]")


def mlp_feature(model, image: torch.Tensor, layer: int, feature: int) -> torch.Tensor:
    """m_b = mean over the patch tokens of GELU unit ``feature`` of vision block ``layer``'s MLP: fp32 [B], differentiable with respect
    to ``image`` ([B, 3, H, W], fp32 or bf16, on the device).  ``model``: a CLIP model or its ``visual`` tower."""
    visual = getattr(model, "visual", model)
    _check_args(visual, image, layer, feature)
    # training's eager front end with the parameters as constants; ln_pre = Identity
    x = _patch_tokens_eager(image, visual.patch_size[0], visual.conv1.weight.detach(), visual.class_embedding.detach(),
                            visual.positional_embedding.detach())
    return _FeatureFn.apply(visual, int(layer), int(feature), x)


class MLPFeatureLoss:
    """``ViTEnsFeatHook(ClipOVGeLUHook(model, sl=slice(layer, layer + 1)), key='high', feat=feature, coefficient)`` with the surface of
    the reference's ``InvLoss`` (cliptoolsoptimized.py:636-654) that ``LossArray`` uses: ``loss(x) = -(1/B^2) sum_b m_b``,
    ``__call__`` returns ``coefficient * loss`` and records ``last_value``."""

    def __init__(self, model, layer: int, feature: int, coefficient: float = 1.0):
        self.model, self.layer, self.f, self.c = model, int(layer), int(feature), coefficient
        self.name = "MLPFeat"
        self.last_value = 0

    def loss(self, x: torch.Tensor) -> torch.Tensor:
        m = mlp_feature(self.model, x, self.layer, self.f)
        return -m.sum() / float(m.shape[0] * m.shape[0])          # -all_feats[:B, f].diag().mean(): a B x B matrix, B^2 entries

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        tensor = self.loss(x)
        self.last_value = tensor.item()
        return self.c * tensor

    def __str__(self) -> str:
        return f"{self.c * self.last_value:.4g}({self.last_value:.4g})"

    def reset(self):
        return 0


# ---- the script's loop on HIP ----------------------------------------------------------------------------------------------------------
SEED = 6247423


def fix_random_seed(seed: int = SEED) -> None:
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def new_init(size: int, batch: int = 1, device="cuda:0") -> torch.Tensor:
    """The script's starting image (cliptoolsoptimized.py:136-150 with its defaults): ``torch.rand(batch, 3, size, size)`` from torch's
    CPU default generator, moved to the device."""
    return torch.rand(batch, 3, size, size).to(device)


def constructor_draws(batch: int, noise_max_iter: int = 400) -> int:
    """The draws the script's augmentation constructors make before the image exists (``ColorJitter.__init__`` and
    ``GaussianNoise.__init__`` each shuffle once: two ``rand`` and one ``randn`` of [batch, 3, 1, 1], one ``rem`` consumed).  The values
    are never used -- every forward shuffles again -- but they advance the generator.  Returns ``rem`` as the first step finds it."""
    torch.rand(batch, 3, 1, 1)
    torch.rand(batch, 3, 1, 1)
    torch.randn(batch, 3, 1, 1)
    return (noise_max_iter - 1 - 1 + noise_max_iter) % noise_max_iter


def draw_tables(steps: int, batch: int, color_mean: float = 1.0, color_std: float = 1.0, noise_std: float = 0.5,
                noise_max_iter: int = 400, jitter: int = 32, rem: int | None = None):
    """Every random draw of ``steps + 1`` iterations, in the script's order, on the host.  Per iteration: ``rand`` (ColorJitter's mean),
    ``rand`` (its std), ``randn`` (GaussianNoise), each [batch, 3, 1, 1] from torch's CPU default generator, then Jitter's two
    ``random.randint(-jitter, jitter)`` from Python's generator:

        mean = (u1 - 0.5) * 2 * color_mean      std = exp((u2 - 0.5) * 2 * color_std)      noise = z * rem * noise_std / noise_max_iter

    in fp32, one operation after the other as torch evaluates the script's expressions; ``rem`` (``noise_max_iter - 1`` unless given)
    then steps down by one modulo ``noise_max_iter``.  Returns (table fp32 [steps + 1, 3, 3 * batch] = mean | std | noise with row b,
    channel c at b * 3 + c; offsets: a list of (off1, off2); the ``rem`` left behind)."""
    rem = noise_max_iter - 1 if rem is None else int(rem)
    table = torch.empty(steps + 1, 3, 3 * batch, dtype=torch.float32)
    offsets = []
    for i in range(steps + 1):
        u1, u2, z = torch.rand(batch, 3, 1, 1), torch.rand(batch, 3, 1, 1), torch.randn(batch, 3, 1, 1)
        table[i, 0] = ((u1 - 0.5) * 2 * color_mean).flatten()
        table[i, 1] = ((u2 - 0.5) * 2 * color_std).exp().flatten()
        table[i, 2] = (z * rem * noise_std / noise_max_iter).flatten()
        rem = (rem - 1 + noise_max_iter) % noise_max_iter
        offsets.append((random.randint(-jitter, jitter), random.randint(-jitter, jitter)))
    return table, offsets, rem


def step_sizes(steps: int, lr: float, beta1: float):
    """clr_i = lr_i / (1 - beta1^(i+1)) with CosineAnnealingLR(T_max = steps, eta_min = 0)'s closed form lr_i = lr (1 + cos(pi i / steps))
    / 2, i = 0 .. steps, in double on the host: what torch.optim.Adamax multiplies exp_avg / exp_inf by at iteration i."""
    return [lr * (1.0 + math.cos(math.pi * i / steps)) / 2.0 / (1.0 - beta1 ** (i + 1)) for i in range(steps + 1)]


class _LoopState:
    """A run's buffers and constants, as ``begin`` of either loop (this one, ``gradient_ascent.GradientAscent``) names them."""


class FeatureVisualizer:
    """The script's ``generate_visualizations`` body for one (layer, feature).  NOTE: constructing one ADVANCES torch's global CPU
    generator (three draws of [repeat * images, 3, 1, 1]), because the script's ColorJitter and GaussianNoise shuffle once in their
    constructors, before ``new_init`` draws the image; that is why ``images`` (N, 1 in the script) is wanted here and not at the call.
    Construct, then ``image = visualizer(new_init(size, images))``.

    ``__call__(image)`` runs ``steps + 1`` iterations on ``image`` ([N, 3, S, S] on the device; not modified) and returns the optimised
    image, fp32 in [0, 1].  ``history`` (device fp32 [steps + 1, 3]) holds (loss, feature_coefficient * -(1/B^2) sum_b m_b,
    tv_coefficient * tv) per iteration; it is read on the host only where a callback asks: ``on_print(i, [loss, feature, tv])`` every
    ``print_every`` iterations, ``on_save(i, image)`` with the image as iteration i found it every ``save_every``.
    ``tv_coefficient`` is the script's ``--tv`` times ``--coeff``.  ``begin(image)`` and ``step(i)`` are the two pieces of ``__call__``;
    with ``debug=True`` a step also keeps ``last_m`` (the objective's m_b) and ``last_grad`` (the gradient the optimiser received)."""

    def __init__(self, model, layer: int, feature: int, steps: int = 400, lr: float = 1.0, tv_coefficient: float = 5e-5,
                 feature_coefficient: float = 1.0, repeat: int = 8, color_mean: float = 1.0, color_std: float = 1.0,
                 noise_std: float = 0.5, noise_max_iter: int = 400, jitter: int = 32, betas=(0.5, 0.99), eps: float = 1e-8,
                 tile: int = 1, images: int = 1, debug: bool = False):
        if int(tile) != 1:
            raise _lib.OvhipError(f"feature visualisation: Tile({tile}) is not built; the script itself runs Tile(1)")
        if steps < 1 or repeat < 1 or noise_max_iter < 1 or jitter < 0:
            raise ValueError("steps, repeat and noise_max_iter must be positive, jitter non-negative")
        self.visual = getattr(model, "visual", model)
        self.layer, self.feature, self.steps, self.lr = int(layer), int(feature), int(steps), float(lr)
        self.c_tv, self.c_feat, self.repeat = float(tv_coefficient), float(feature_coefficient), int(repeat)
        self.aug_args = dict(color_mean=color_mean, color_std=color_std, noise_std=noise_std, noise_max_iter=int(noise_max_iter),
                             jitter=int(jitter))
        self.betas, self.eps, self.debug = (float(betas[0]), float(betas[1])), float(eps), bool(debug)
        self.history = self.last_m = self.last_grad = None
        self.images = int(images)                   # N: the script builds ColorJitter(8) / GaussianNoise(8) for RepeatBatch(8) of one image
        self._rem = constructor_draws(self.repeat * self.images, self.aug_args["noise_max_iter"])
        self._s = None

    def begin(self, image: torch.Tensor) -> None:
        """Checks, the run's host draws and their one upload, every buffer of the loop."""
        visual = self.visual
        _check_args(visual, image, self.layer, self.feature)
        lib = _lib.load()
        n, _, size, width = image.shape
        p = visual.patch_size[0]
        if size != width or size % p:
            raise ValueError(f"image must be square with a side that is a multiple of the patch size {p}")
        if n != self.images:
            raise ValueError(f"built for images={self.images} (the augmentations' batch is repeat * images), got {n}")
        g = size // p
        grid, batch = g * g, self.repeat * n
        pos = visual.positional_embedding.detach().float().contiguous()
        if pos.shape[0] != 1 + grid:
            raise ValueError(f"the tower's positional embedding has {pos.shape[0]} rows; a {size} x {size} image needs {1 + grid}")
        d = pos.shape[1]
        dev = image.device
        s = _LoopState()
        s.n, s.size, s.p, s.grid, s.batch, s.d, s.seq = n, size, p, grid, batch, d, 1 + grid
        s.kp, s.npad = _round_up(3 * p * p, 64), _round_up(d, 64)
        table, s.offsets, self._rem = draw_tables(self.steps, batch, rem=self._rem, **self.aug_args)
        s.table = table.to(dev)
        s.clr = step_sizes(self.steps, self.lr, self.betas[0])
        w = visual.conv1.weight.detach()
        s.w = _pack_matrix(w.reshape(w.shape[0], -1), s.npad, s.kp)
        s.cls, s.pos = visual.class_embedding.detach().float().contiguous(), pos
        s.keep = torch.arange(grid, dtype=torch.int32, device=dev).repeat(batch, 1).contiguous()      # every patch, in order: its own inverse
        s.dm = (-(torch.tensor(self.c_feat, dtype=torch.float32, device=dev) / float(batch * batch))).expand(batch).contiguous()
        rows = batch * grid
        new = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        s.img = image.detach().float().contiguous().clone()
        s.cols, s.dcols = new(rows, s.kp, dtype=torch.bfloat16), new(rows, s.kp, dtype=torch.bfloat16)
        s.y, s.dy = new(rows, s.npad, dtype=torch.bfloat16), new(rows, s.npad, dtype=torch.bfloat16)
        s.aug, s.norms = new(batch, 3, size, size), new(4, 3 * batch)
        s.x32, s.dxf = new(batch, s.seq, d), new(batch, s.seq, d)
        s.xb = new(batch, s.seq, d, dtype=torch.bfloat16)
        s.dimg, s.ea, s.ei = new(n, 3, size, size), new(n, 3, size, size), new(n, 3, size, size)
        s.ws_bytes = lib.ov_linear_backward_workspace_bytes(rows, s.npad, s.kp)
        s.ws = torch.empty(s.ws_bytes + 256, dtype=torch.uint8, device=dev)
        self.history = new(self.steps + 1, 3)
        self._s = s

    def step(self, i: int) -> None:
        """Iteration i (0 .. steps) of the run ``begin`` prepared: launches only."""
        lib, s, st = _lib.load(), self._s, stream_ptr()
        n, r, size, p, grid, batch, d, kp = s.n, self.repeat, s.size, s.p, s.grid, s.batch, s.d, s.kp
        tokens = batch * s.seq
        off1, off2 = s.offsets[i]
        table = C.c_void_p(s.table.data_ptr() + i * 9 * batch * 4)
        check(lib.ov_viz_augment(ptr(s.img), table, n, r, size, p, kp, off1, off2, ptr(s.cols), ptr(s.aug), st), "ov_viz_augment")
        # mlp_feature's front end on the same operand rows: y = cols W^T (bf16), x = [cls; y] + pos in fp32, then the bf16 tokens
        _patch_tokens_forward(s.cols, s.w, s.cls, s.pos, s.keep, grid, s.y, s.x32, st)
        check(lib.ov_convert(ptr(s.x32), _lib.OV_F32, d, ptr(s.xb), _lib.OV_BF16, d, tokens, d, st), "ov_convert")
        m, state = _feature_forward(self.visual, self.layer, self.feature, s.xb, True)
        check(lib.ov_viz_tv(ptr(s.aug), batch, size, size, ptr(s.norms), None, st), "ov_viz_tv")
        dx = _feature_backward(state, s.dm)
        # back through the bf16 tokens, the fp32 assembly (the patch rows only) and the projection: dcols, nothing for the weight
        check(lib.ov_convert(ptr(dx), _lib.OV_BF16, d, ptr(s.dxf), _lib.OV_F32, d, tokens, d, st), "ov_convert")
        _patch_tokens_backward(s.dxf, s.keep, grid, s.dy, s.w, s.ws, s.ws_bytes, st, dcols=s.dcols)
        row = C.c_void_p(self.history.data_ptr() + i * 12)
        check(lib.ov_viz_augment_backward(ptr(s.dcols), kp, ptr(s.aug), ptr(s.norms), table, ptr(m), n, r, size, p, off1, off2, size,
                                          self.c_feat, self.c_tv, ptr(s.dimg), row, st), "ov_viz_augment_backward")
        if self.debug:
            self.last_m, self.last_grad = m.clone(), s.dimg.clone()
        check(lib.ov_adamax_clip_step(ptr(s.img), ptr(s.dimg), ptr(s.ea), ptr(s.ei), s.img.numel(), s.clr[i], self.betas[0], self.betas[1],
                                      self.eps, 0.0, 1.0, st), "ov_adamax_clip_step")

    @property
    def image(self) -> torch.Tensor:
        """The image as the last step left it."""
        return self._s.img

    def __call__(self, image: torch.Tensor, print_every: int = 0, on_print=None, save_every: int = 0, on_save=None) -> torch.Tensor:
        self.begin(image)
        for i in range(self.steps + 1):
            if save_every and on_save is not None and i % save_every == 0:
                on_save(i, self._s.img)
            self.step(i)
            if print_every and on_print is not None and i % print_every == 0:
                on_print(i, self.history[i].tolist())
        return self._s.img
