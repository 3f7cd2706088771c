"""Counterpart of the fork's ``ov-gradient-ascent.py`` on the MI355X path: the text "opinion" of a CLIP model about one image.

    python -m openvision_amd.gradient_ascent --use_model DIR --use_image FILE [--img_folder DIR] [--batch_size 13] [--deterministic]
        [--steps 340] [--tokens 4]

The script learns ``normu`` fp32 [B, K, V] -- B = 13 samples of K = 4 token distributions -- for 340 iterations of
(ov-gradient-ascent.py:226-259, :380-381)

    img    = Normalization(RandomAffine(10, translate=.1, p=.8)(image expanded to B))      ov_ga_affine, then model.encode_image (no_grad)
    soft   = F.gumbel_softmax(normu, tau=1000, hard=True)                                  ov_ga_sample: idx = argmax (normu - log e) / tau
    tx     = text tower(cat(prompt, pad, soft) @ W + pos)                                  a row gather of W at the ids, then
                                                                                           training.encode_text_embeddings, input-only
    loss   = mean_j -100 mean_i cos(tx_j, img_i)                                           ov_ga_cosine_loss (forward, d tx, best so far)
    normu  = Adam(lr=5)(normu, d loss / d normu)                                           ov_ga_token_grad + ov_ga_adam

``GradientAscent`` is that loop as launches.  The forward value of ``soft`` is a one-hot row, so the tower's input at a learned
position is ``W[idx]`` and the ``[B, 80, V] @ [V, D]`` product of the script is a gather; the backward needs the gradient dX at the K
learned positions only, and d normu = ys (dX W^T - c) / tau is formed from it without a ``[B, 80, V]`` tensor.  A step makes no
host-to-device copy, no ``.item()`` and no host synchronisation: the best loss, its step and its text embedding are tracked on the
device, every sampled index goes to a device history, and ``checkin`` rebuilds the script's printed "bests" from the two histories
where a print is asked for.

Departures from the script, both deliberate:
  * its ``GradScaler`` / ``autocast`` pair is fp16 underflow protection around an fp32 model (``scaler.step`` unscales before Adam sees
    the gradient); the towers here run bf16, which has fp32's exponent range, so neither is reproduced;
  * kornia is not a dependency of this package, so the ORDER in which ``kornia.augmentation.RandomAffine`` draws its parameters
    cannot be pinned.  ``draw_affine`` draws the same distributions (apply with probability p; angle U(-degrees, degrees); translation
    U(-translate S, translate S) per axis) from torch's CPU generator, in double, in its own documented order.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
from typing import List, Optional, Sequence

import torch
import torch.nn.functional as F

from . import _lib, config as ovcfg, training
from ._lib import check, ptr, stream_ptr
from .visualize import _LoopState, fix_random_seed

__all__ = ["GradientAscent", "draw_affine", "inverse_matrices", "affine_theta", "checkin", "mean_loss", "load_image", "main"]

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".tiff", ".gif")


# ---- the host draws ----------------------------------------------------------------------------------------------------------------------
def inverse_matrices(apply: torch.Tensor, angle_deg: torch.Tensor, tx: torch.Tensor, ty: torch.Tensor, size: int) -> torch.Tensor:
    """The inverse pixel maps (destination -> source) of 'rotate by angle about the image centre, then translate by (tx, ty)', in
    double: [..., 6] = (a0, a1, a2, a3, a4, a5) with sx = a0 x + a1 y + a2, sy = a3 x + a4 y + a5.  The centre is ((S - 1) / 2,
    (S - 1) / 2) in pixel indices; rows where ``apply`` is false hold the identity exactly."""
    a = angle_deg.double() * (math.pi / 180.0)
    c, s = torch.cos(a), torch.sin(a)
    ctr = (size - 1) / 2.0
    # forward p' = R (p - ctr) + ctr + t with R = [[c, -s], [s, c]]; inverse p = R^T (p' - ctr - t) + ctr
    ox, oy = ctr + tx.double(), ctr + ty.double()
    m = torch.stack([c, s, ctr - (c * ox + s * oy), -s, c, ctr - (-s * ox + c * oy)], dim=-1)
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64).expand_as(m)
    return torch.where(apply.unsqueeze(-1), m, ident)


def draw_affine(steps: int, batch: int, size: int, degrees: float = 10.0, translate: float = 0.1, p: float = 0.8):
    """Every affine parameter of a run, on the host, in double, from torch's CPU default generator: ONE ``torch.rand(steps, batch, 4,
    dtype=float64)``, per (step, sample) u0 -> apply = u0 < p, u1 -> angle = (2 u1 - 1) degrees, u2 / u3 -> tx / ty = (2 u - 1)
    translate S.  (kornia's own draw order is not reproduced: see the module docstring.)  Returns (mats fp32 [steps, batch, 6] -- the
    inverse pixel maps ov_ga_affine reads -- and params float64 [steps, batch, 4] = apply, angle, tx, ty)."""
    u = torch.rand(steps, batch, 4, dtype=torch.float64)
    apply = u[..., 0] < p
    angle = (2.0 * u[..., 1] - 1.0) * degrees
    tx = (2.0 * u[..., 2] - 1.0) * (translate * size)
    ty = (2.0 * u[..., 3] - 1.0) * (translate * size)
    mats = inverse_matrices(apply, angle, tx, ty, size).float()
    return mats, torch.stack([apply.double(), angle, tx, ty], dim=-1)


def affine_theta(mats: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """``F.affine_grid``'s theta [..., 2, 3] (normalised coordinates, align_corners=False) of the inverse pixel maps [..., 6]."""
    a0, a1, a2, a3, a4, a5 = mats.unbind(-1)
    h, w = float(height), float(width)
    r0 = torch.stack([a0, a1 * h / w, a0 + a1 * h / w - (a0 + a1) / w + (2 * a2 + 1) / w - 1], dim=-1)
    r1 = torch.stack([a3 * w / h, a4, a3 * w / h + a4 - (a3 + a4) / h + (2 * a5 + 1) / h - 1], dim=-1)
    return torch.stack([r0, r1], dim=-2)


# ---- the script's book-keeping, from the histories ---------------------------------------------------------------------------------------
def mean_loss(history: torch.Tensor) -> torch.Tensor:
    """mean_j loss1[j] per step as ov_ga_cosine_loss forms it: fp32, j ascending, then one division.  history [steps, B] -> [steps]."""
    import numpy as np
    h = history.detach().float().cpu().numpy()
    s = np.zeros(h.shape[:-1], dtype=np.float32)
    for j in range(h.shape[-1]):                        # float32 + float32: one rounding per addition, as on the device
        s = s + h[..., j]
    return torch.from_numpy(np.asarray(s / np.float32(h.shape[-1]), dtype=np.float32))


def _strip_punctuation(text: str) -> str:
    for ch in ".;_-\\'\"^&#)(,":
        text = text.replace(ch, "")
    return text


def checkin(ids_history: torch.Tensor, history: torch.Tensor, tokenizer, name: str, upto: Optional[int] = None, every: int = 50,
            out_dir: Optional[str] = "opinion-tokens", log=None):
    """The script's ``bests`` dictionary after iterations [0, upto) (ov-gradient-ascent.py:156-193, :279-293), rebuilt on the host from
    ``ids_history`` (int [steps, B, K]) and ``history`` (fp32 [steps, B]): the script calls its ``checkin`` at every new best mean
    loss and every ``every`` iterations, and each call moves the samples whose loss beats the worst kept entry into ``bests``.
    Returns the list of (loss, text) in the dictionary's order; the unique words of its first five texts, punctuation stripped, go to
    ``{out_dir}/tokens_{name}.txt`` (sorted: the script joins a set).  ``log(line)`` receives what the script prints."""
    ids = ids_history.detach().cpu()
    hist = history.detach().float().cpu()
    means = mean_loss(hist)
    upto = ids.shape[0] if upto is None else min(int(upto), ids.shape[0])
    bests = [[1000.0 + k, "None"] for k in range(6)]
    best = float("inf")

    def visit(j):
        texts = [tokenizer.decode(ids[j, b].tolist(), skip_special_tokens=True, clean_up_tokenization_spaces=True)
                 for b in range(ids.shape[1])]
        for b, text in enumerate(texts):
            loss = float(hist[j, b])
            if loss < max(k for k, _ in bests):
                bests.append([loss, "".join(c if c.isprintable() else " " for c in text)])
                worst = max(k for k, _ in bests)
                bests.pop(max(i for i, (k, _) in enumerate(bests) if k == worst))
                if log is not None:
                    log(f"Sample {b} Tokens: " + "".join(c for c in text if c.isprintable()))

    for j in range(upto):
        cur = float(means[j])
        if cur < best:
            best = cur
            if log is not None:
                log(f"New best loss: {best:.3f}")
            visit(j)
        if every and j % every == 0:
            if log is not None:
                log(f"Iteration {j}: Average Loss: {cur:.3f}")
            visit(j)
    if out_dir is not None:
        words = set()
        for _, text in bests[:5]:
            words.update(_strip_punctuation(text).split())
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"tokens_{name}.txt"), "w", encoding="utf-8") as f:
            f.write(" ".join(sorted(words)))
    return [(k, t) for k, t in bests]


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
class GradientAscent:
    """The script's ``generate_target_text_embeddings`` body for one image.  ``begin(image)`` draws every affine parameter of the run
    on the host (``draw_affine``: torch's CPU generator, in double; kornia's own draw order cannot be pinned, it is not a dependency)
    and ``normu`` as ``torch.zeros(B, K, V).normal_()`` as the script's ``Pars`` does, uploads both once, allocates every buffer and
    freezes the model's parameters (the text tower then runs its input-only backward); ``step(i)`` is launches only; ``end()`` puts the
    ``requires_grad`` flags back.  ``__call__(image)`` is the three together and returns ``best_text_embedding``.

    ``image``: [3, S, S] or [1, 3, S, S] in [0, 1] on the device, S the model's image size.  ``prompt``: token ids in front of the
    padding (the script's is empty).  Results: ``history`` (device fp32 [steps, B], loss1 per sample), ``ids_history`` (device int32
    [steps, B, K], the sampled ids), ``best_loss`` / ``best_step`` / ``best_text_embedding`` (read from the device where asked for),
    ``normu``; with ``debug=True`` a step also keeps ``last_grad`` (d loss / d normu as Adam received it, [B, K, V]), ``last_dx`` (the
    bf16 gradient rows at the learned positions, [B K, D]), ``last_x`` / ``last_xgrad`` (the tower's input and its whole gradient),
    ``last_tx`` and ``last_img`` (the two towers' features).
    ``on_print(i, mean loss)`` is called every ``print_every`` iterations and synchronises; nothing else does."""

    def __init__(self, model, batch_size: int = 13, tokens: int = 4, steps: int = 340, lr: float = 5.0, tau: float = 1000.0,
                 betas=(0.9, 0.999), eps: float = 1e-8, degrees: float = 10.0, translate: float = 0.1, p: float = 0.8,
                 prompt: Sequence[int] = (), pad_token_id: int = 0, mean=ovcfg.DEFAULT_PREPROCESS["mean"],
                 std=ovcfg.DEFAULT_PREPROCESS["std"], debug: bool = False):
        if batch_size < 1 or tokens < 1 or steps < 1:
            raise ValueError("batch_size, tokens and steps must be positive")
        if not tau > 0 or not 0 <= p <= 1:
            raise ValueError("tau must be positive and p a probability")
        self.model = model
        self.batch, self.k, self.steps, self.lr, self.tau = int(batch_size), int(tokens), int(steps), float(lr), float(tau)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.degrees, self.translate, self.p = float(degrees), float(translate), float(p)
        self.prompt, self.pad = [int(t) for t in prompt], int(pad_token_id)
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        self.debug = bool(debug)
        self.history = self.ids_history = self.normu = None
        self.last_grad = self.last_dx = self.last_x = self.last_xgrad = self.last_tx = self.last_img = None
        self._s = self._flags = None

    # -- set-up and tear-down ------------------------------------------------------------------------------
    def begin(self, image: torch.Tensor) -> None:
        """Checks, the run's host draws and their one upload, every buffer of the loop; freezes the model's parameters."""
        model, lib = self.model, _lib.load()
        if not image.is_cuda:
            raise _lib.OvhipError("gradient ascent: tensors must live on an MI355X device (no CPU fallback)")
        if image.dim() == 4 and image.shape[0] == 1:
            image = image[0]
        if image.dim() != 3 or image.shape[0] < 3 or image.shape[1] != image.shape[2]:
            raise ValueError("image must be one square image, [3, S, S] or [1, 3, S, S]")
        size = image.shape[1]
        if size != model.visual.image_size[0]:
            raise ValueError(f"the model takes {model.visual.image_size[0]} x {model.visual.image_size[0]} images, got {size}")
        w = model.token_embedding.weight
        vocab, d = w.shape
        t = int(model.context_length)
        b, k = self.batch, self.k
        if k + len(self.prompt) > t:
            raise ValueError(f"{len(self.prompt)} prompt and {k} learned tokens do not fit a context of {t}")
        if any(not 0 <= i < vocab for i in self.prompt + [self.pad]):
            raise ValueError("prompt / pad token ids outside the vocabulary")
        if d % 64:
            raise _lib.OvhipError("gradient ascent: the text width must be a multiple of 64")
        if b > 64:
            raise _lib.OvhipError("gradient ascent: batch_size <= 64 (ov_ga_cosine_loss runs in one workgroup)")
        dev = image.device
        s = _LoopState()
        s.size, s.vocab, s.d, s.t, s.r, s.e = size, vocab, d, t, b * k, int(model.embed_dim)
        mats, s.params = draw_affine(self.steps, b, size, self.degrees, self.translate, self.p)
        s.mats = mats.to(dev)
        self.normu = torch.zeros(b, k, vocab).normal_().to(dev)
        new = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        s.img = image[:3].detach().float().contiguous().clone()
        s.mean, s.std = torch.tensor(self.mean, device=dev), torch.tensor(self.std, device=dev)
        s.aug = new(b, 3, size, size)
        s.ids = torch.tensor(self.prompt + [self.pad] * (t - len(self.prompt)), dtype=torch.int64).repeat(b, 1).to(dev)
        s.idx, s.zmax, s.zsum, s.z = new(s.r, dtype=torch.int32), new(s.r), new(s.r), new(s.r, vocab)
        s.nblk = lib.ov_ga_parts_blocks(vocab)
        s.gy, s.parts = new(s.r, vocab), new(s.r, s.nblk)
        s.ea, s.es = new(s.r, vocab), new(s.r, vocab)
        s.g = new(s.r, vocab) if self.debug else None
        s.dtx, s.best_tx = new(b, s.e), new(b, s.e)
        s.best = torch.full((1,), float("inf"), dtype=torch.float32, device=dev)
        s.best_step = torch.full((1,), -1, dtype=torch.int32, device=dev)
        s.w32 = w.detach().float()                        # the table training.encode_text gathers from (the weight itself when fp32)
        s.wb = model.token_embedding.packed()             # the bf16 table the text front end holds: ov_ga_token_grad's W
        s.argmax_pool = getattr(model, "text_pool_type", "last") == "argmax"
        self.history = new(self.steps, b)
        self.ids_history = new(self.steps, b, k, dtype=torch.int32)
        self._flags = [(q, q.requires_grad) for q in model.parameters()]
        for q, _ in self._flags:
            q.requires_grad_(False)
        self._s = s

    def end(self) -> None:
        """Puts the parameters' ``requires_grad`` flags back as ``begin`` found them."""
        if self._flags is not None:
            for q, flag in self._flags:
                q.requires_grad_(flag)
            self._flags = None

    # -- one iteration -------------------------------------------------------------------------------------
    def step(self, i: int) -> None:
        """Iteration i (0 .. steps - 1) of the run ``begin`` prepared: launches only."""
        lib, s, st, model = _lib.load(), self._s, stream_ptr(), self.model
        b, k, r, vocab, d, t, e = self.batch, self.k, s.r, s.vocab, s.d, s.t, s.e
        normu = self.normu
        mats = C.c_void_p(s.mats.data_ptr() + i * b * 6 * 4)
        check(lib.ov_ga_affine(ptr(s.img), mats, ptr(s.mean), ptr(s.std), ptr(s.aug), _lib.OV_F32, b, s.size, st), "ov_ga_affine")
        with torch.no_grad():
            feats = model.encode_image(s.aug, normalize=False).float().contiguous()
        noise = torch.empty(r, vocab, dtype=torch.float32, device=normu.device).exponential_()      # F.gumbel_softmax's own draw
        hist_ids = C.c_void_p(self.ids_history.data_ptr() + i * r * 4)
        check(lib.ov_ga_sample(ptr(normu), ptr(noise), self.tau, r, vocab, k, t, ptr(s.z), ptr(s.idx), ptr(s.zmax), ptr(s.zsum), hist_ids,
                               ptr(s.ids), st), "ov_ga_sample")
        x = F.embedding(s.ids, s.w32).requires_grad_(True)                  # W[ids]: what `tokens @ W` is for one-hot rows
        pool_index = s.ids.argmax(dim=-1) if s.argmax_pool else None
        tx = training.encode_text_embeddings(model, x, normalize=False, pool_index=pool_index)
        txc = tx.detach().float().contiguous()
        row = C.c_void_p(self.history.data_ptr() + i * b * 4)
        check(lib.ov_ga_cosine_loss(ptr(txc), ptr(feats), b, e, i, row, ptr(s.dtx), ptr(s.best), ptr(s.best_step), ptr(s.best_tx), st),
              "ov_ga_cosine_loss")
        tx.backward(s.dtx.to(tx.dtype))
        dx = x.grad[:, t - k:, :].to(torch.bfloat16).reshape(r, d).contiguous()      # the tower's backward is bf16: this cast is exact
        check(lib.ov_ga_token_grad(ptr(dx), ptr(s.wb), ptr(s.z), ptr(s.zmax), ptr(s.zsum), r, vocab, d, ptr(s.gy), ptr(s.parts), st),
              "ov_ga_token_grad")
        if self.debug:
            self.last_dx, self.last_x, self.last_tx, self.last_img = dx, x.detach(), txc, feats
            self.last_xgrad = x.grad
        n = i + 1
        check(lib.ov_ga_adam(ptr(s.gy), ptr(s.parts), ptr(normu), ptr(s.z), ptr(s.zmax), ptr(s.zsum), self.tau, r, vocab, ptr(s.ea),
                             ptr(s.es), self.lr, self.betas[0], self.betas[1], self.eps, 1.0 - self.betas[0] ** n, 1.0 - self.betas[1] ** n,
                             ptr(s.g), st), "ov_ga_adam")
        if self.debug:
            self.last_grad = s.g.view(b, k, vocab).clone()

    # -- results -------------------------------------------------------------------------------------------
    @property
    def best_loss(self) -> float:
        return float(self._s.best.item())

    @property
    def best_step(self) -> int:
        return int(self._s.best_step.item())

    @property
    def best_text_embedding(self) -> torch.Tensor:
        return self._s.best_tx

    def __call__(self, image: torch.Tensor, print_every: int = 0, on_print=None) -> torch.Tensor:
        self.begin(image)
        try:
            for i in range(self.steps):
                self.step(i)
                if print_every and on_print is not None and i % print_every == 0:
                    on_print(i, float(mean_loss(self.history[i])))
        finally:
            self.end()
        return self._s.best_tx


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def load_image(img_path: str, side_x: int, side_y: int, device="cuda:0") -> torch.Tensor:
    """ov-gradient-ascent.py:73-76: RGB, / 255, nearest ``F.interpolate`` to (side_x, side_y).  [1, 3, side_x, side_y] fp32."""
    import numpy as np
    from PIL import Image
    im = torch.tensor(np.array(Image.open(img_path).convert("RGB"))).to(device).unsqueeze(0).permute(0, 3, 1, 2) / 255
    return F.interpolate(im, (side_x, side_y))


def parse_arguments(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(description="OpenVision gradient ascent (MI355X)")
    ap.add_argument("--batch_size", default=13, type=int)
    ap.add_argument("--use_model", default="openvision-vit-large-patch14-224", help="Path to an OpenVision model")
    ap.add_argument("--use_image", type=str, default="testcat/catdog.png", help="Path to image")
    ap.add_argument("--img_folder", type=str, default="None", help="Path to image folder (batch process)")
    ap.add_argument("--deterministic", action="store_true", help="Use deterministic behavior (torch, numpy, random seeds)")
    ap.add_argument("--steps", default=340, type=int, help="optimisation steps per image (the script's `iterations`)")
    ap.add_argument("--tokens", default=4, type=int, help="learned tokens per sample (the script's `tokinit`)")
    return ap.parse_args(argv)


def image_paths(args) -> List[str]:
    if args.img_folder != "None":
        return [os.path.join(args.img_folder, f) for f in sorted(os.listdir(args.img_folder)) if f.lower().endswith(IMAGE_EXTENSIONS)]
    return [args.use_image]


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_arguments(argv)
    from .checkpoint import from_pretrained
    from .tokenizer import WordPieceTokenizer, clean
    if args.deterministic:
        fix_random_seed()
    model, pp = from_pretrained(args.use_model, device="cuda:0")
    size = model.visual.image_size[0]
    vocab_file = os.path.join(args.use_model, "vocab.txt")
    tok = WordPieceTokenizer(vocab_file if os.path.exists(vocab_file) else None, context_length=model.context_length)
    prompt = [i for i in tok.encode(clean("")) if i not in (0, 100, 101, 102, 103)]           # the script's empty prompt, specials dropped
    for path in image_paths(args):
        name = os.path.splitext(os.path.basename(path))[0]
        print(f"\nRunning gradient ascent for {name}...\n", flush=True)
        ga = GradientAscent(model, batch_size=args.batch_size, tokens=args.tokens, steps=args.steps, prompt=prompt, mean=pp["mean"],
                            std=pp["std"])
        shown = [0]

        def show(i, mean, ga=ga, name=name, shown=shown):
            lines = []
            checkin(ga.ids_history, ga.history, tok, name, upto=i + 1, log=lines.append)
            print("\n".join(lines[shown[0]:]), flush=True)
            shown[0] = len(lines)

        best_tx = ga(load_image(path, size, size), print_every=50, on_print=show)
        show(args.steps - 1, None)
        os.makedirs("txtembeds", exist_ok=True)
        torch.save(best_tx.detach().clone(), f"txtembeds/{name}_text_embedding.pt")
        print(f"Best loss {ga.best_loss:.3f} at iteration {ga.best_step}.\nBest text embedding saved to 'txtembeds'.\n"
              "Tokens (CLIP 'opinion') saved to 'opinion-tokens' folder.\n", flush=True)
        print(f"Done processing image: {path}", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
