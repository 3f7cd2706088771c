"""CPU: the one statement of the gathered-side gradient routing (openvision_amd.loss.route_gradient) on two gloo ranks against the
sums written out, and the two layouts of the gathered-gradient buffer (openvision_amd.loss.gathered_gradient_buffer) element by
element.  The three InfoNCE-type backwards (ClipLoss / MultiCaptionClipLoss / DistillClipLoss) call exactly these two."""
import pytest
import torch

from openvision_amd import loss as L

from ranks import run_ranks

WS, B, E = 2, 3, 8
WIDTHS = (2 * E, 3 * E)                     # ClipLoss / DistillClipLoss's student half, and two caption sets
MODES = [(True, False), (True, True), (False, False), (False, True)]          # (local_loss, gather_with_grad)


def _grads(w):
    """Hand-made packed gradients that differ on every rank: per rank the local side of its own rows [b, W], the local side of the
    global loss [N, W], and the gathered side [N, W]."""
    g = torch.Generator().manual_seed(7 + w)
    loc = [torch.randn(B, w, generator=g) for _ in range(WS)]
    glo = [torch.randn(WS * B, w, generator=g) for _ in range(WS)]
    gat = [torch.randn(WS * B, w, generator=g) for _ in range(WS)]
    return loc, glo, gat


def _gloo_rank(rank, ws):
    out = {}
    for w in WIDTHS:
        loc, glo, gat = _grads(w)
        for local_loss, gwg in MODES:
            d_local = (loc if local_loss else glo)[rank].clone()
            d_gathered = None if local_loss and not gwg else gat[rank].clone()      # a detached gather under local_loss carries none
            out[(w, local_loss, gwg)] = L.route_gradient(d_local, d_gathered, B, rank, True, local_loss, gwg)
            # no collective: the flags do not matter, both sides are the same [b, W] rows
            out[(w, local_loss, gwg, "single")] = L.route_gradient(loc[rank].clone(), gat[rank][:B].clone(), B, rank, False,
                                                                   local_loss, gwg)
    # plain arrays on the queue: a tensor travels as a shared file descriptor, which needs this process alive when the parent reads
    return {k: v.numpy().copy() for k, v in out.items()}


def test_route_gradient_in_every_mode_over_gloo():
    """Two gloo ranks on CPU tensors, b = 3, W = 2 E and 3 E: what route_gradient returns on each rank in the four collective modes
    and without a collective, against the sums it stands for."""
    res = [{k: torch.from_numpy(v) for k, v in out.items()} for out in run_ranks(_gloo_rank, WS, timeout=300, backend="gloo")]
    for w in WIDTHS:
        loc, glo, gat = _grads(w)
        for rank in range(WS):
            out, own = res[rank], slice(rank * B, (rank + 1) * B)
            for local_loss, gwg in MODES:
                single = out[(w, local_loss, gwg, "single")]
                assert single.shape == (B, w) and torch.allclose(single, loc[rank] + gat[rank][:B])
                assert out[(w, local_loss, gwg)].shape == (B, w)
            assert torch.equal(out[(w, True, False)], loc[rank])
            assert torch.allclose(out[(w, True, True)], loc[rank] + sum(gat)[own])
            assert torch.equal(out[(w, False, False)], (glo[rank] + gat[rank])[own])
            assert torch.allclose(out[(w, False, True)], sum(g_ + a_ for g_, a_ in zip(glo, gat))[own])
            assert not torch.equal(out[(w, True, True)], out[(w, True, False)])           # the ranks' terms differ: a sum is visible


@pytest.mark.parametrize("c", [1, 3])
def test_gathered_gradient_buffer_layouts_address_the_same_elements(c):
    """Both layouts of the gathered-gradient buffer, written the way a kernel addresses them (pointer, ldg, gset_stride) and read
    as tensors (the packed one through unpack_caption_features), and the other way round: every element is addressed exactly once
    and (part, set, row, column) lands where the routing reads it."""
    n, e = 5, E
    img = torch.arange(n * e, dtype=torch.float32).view(n, e)
    txt = 1000.0 + torch.arange(c * n * e, dtype=torch.float32).view(c * n, e)
    rows, cols = torch.meshgrid(torch.arange(n), torch.arange(e), indexing="ij")
    for packed in (False, True):
        buf, p_img, p_txt, ldg, gss = L.gathered_gradient_buffer(n, e, c, packed, "cpu")
        assert buf.shape == ((n, (1 + c) * e) if packed else ((1 + c) * n, e)) and buf.dtype == torch.float32 and buf.is_contiguous()
        assert (ldg, gss) == (((1 + c) * e, e) if packed else (e, n * e))
        flat = buf.view(-1)
        off_i, off_t = (p_img.value - buf.data_ptr()) // 4, (p_txt.value - buf.data_ptr()) // 4
        assert off_i == 0 and off_t == (e if packed else n * e)

        def read(tensors):
            return L.unpack_caption_features(tensors, c) if packed else (tensors[:n], tensors[n:])

        flat.fill_(float("nan"))
        flat[off_i + ldg * rows + cols] = img
        for k in range(c):
            flat[off_t + k * gss + ldg * rows + cols] = txt[k * n:(k + 1) * n]
        assert not bool(torch.isnan(buf).any())
        got_img, got_txt = read(buf)
        assert torch.equal(got_img, img) and torch.equal(got_txt, txt)
        # the other way round: written as tensors, read by the kernel's arithmetic
        buf.copy_(L.pack_caption_features(img + 0.5, txt + 0.5, c) if packed else torch.cat([img + 0.5, txt + 0.5]))
        assert torch.equal(flat[off_i + ldg * rows + cols], img + 0.5)
        for k in range(c):
            assert torch.equal(flat[off_t + k * gss + ldg * rows + cols], txt[k * n:(k + 1) * n] + 0.5)
