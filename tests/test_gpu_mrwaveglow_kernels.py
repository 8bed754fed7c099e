"""The kernels of csrc/wg_mr.h one by one on the MI355X (-m gpu), through the C ABI on buffers of the test's own: every buffer a kernel
writes is pre-filled with NaN, so an element it does not own must come back NaN and one it owns must not.

  * Haar split / merge and their backward modes: bit-equal to fp32 torch on the CPU -- every output is one rounding of exact operands
    (a multiplication by 1/2 is exact), so neither an fma nor the order of the operations can change it;
  * the upsampling and its backward against float64 F.interpolate and its autograd, each element within the project's fp32 fma-chain
    bound (n + 3) 2^-24 sum |a_i b_i| (2 terms forward, at most 2s backward); frames no column reads get exactly 0;
  * pack / unpack: bit-equal;
  * a second run of every backward repeats the first bit for bit.

T in {8, 260} and the misaligned cases are there for the 16-byte paths, which need T % 4 == 0 and aligned rows."""
import itertools

import pytest
import torch

import fill
import mr_ref64 as r64
from constant_memory_waveglow_amd import _lib, engine
from constant_memory_waveglow_amd._lib import check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")


def dev(name, shape, pad=0):
    """deterministic values on the device; pad: elements the tensor is shifted by inside its storage (pad = 1 breaks 16-byte alignment)"""
    t = torch.from_numpy(fill.normal(name, shape))
    if not pad:
        return t.to(DEV)
    buf = torch.empty(t.numel() + pad, device=DEV)
    buf[pad:] = t.reshape(-1).to(DEV)
    return buf[pad:].view(shape)


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def split(x, mode, diff, avg, cond):
    B, c, T = x.shape
    check(_lib.lib().wg_mr_haar_split(engine._p(x), x.stride(0), x.stride(1), x.stride(2), B, c, T, mode, engine._p(diff), engine._p(avg),
                                      engine._p(cond), 0 if cond is None else cond.size(1), engine._stream(DEV)), "wg_mr_haar_split")


def merge(avg, diff, mode, out, avg2=None):
    B, half, T = avg.shape
    check(_lib.lib().wg_mr_haar_merge(engine._p(avg), engine._p(avg2), 0 if avg2 is None else avg2.size(1), engine._p(diff), B, 2 * half, T,
                                      mode, engine._p(out), out.stride(0), out.stride(1), out.stride(2), engine._stream(DEV)),
          "wg_mr_haar_merge")


def layouts(B, c, T, fill_with=None):
    """[B, c, T] tensors in the layouts the kernels take: contiguous, the audio's [B, T, c], the same inside wider rows (elements between
    the rows belong to nobody), and contiguous but shifted off 16-byte alignment"""
    def make(shape):
        return nans(*shape) if fill_with is None else dev(fill_with, shape)
    out = {"contiguous": make((B, c, T)), "channels_last": make((B, T, c)).transpose(1, 2),
           "padded": make((B, T, c + 3))[:, :, :c].transpose(1, 2)}
    if fill_with is None:
        out["shifted"] = nans(B * c * T + 1)[1:].view(B, c, T)
    else:
        out["shifted"] = dev(fill_with, (B, c, T), pad=1)
    return out


HAAR = list(itertools.product([2, 4, 8, 16], [1, 7, 33, 257, 8, 260]))


@pytest.mark.parametrize("c,T", HAAR)
def test_haar_split_is_bit_equal(c, T):
    for B, mode in itertools.product([1, 3], [0, 1]):
        a, b = (1.0, 0.5) if mode == 0 else (0.5, 1.0)
        for name, x in layouts(B, c, T, "haar/x%d" % c).items():
            xc = x.cpu()
            want_diff, want_avg = a * (xc[:, 1::2] - xc[:, ::2]), b * (xc[:, ::2] + xc[:, 1::2])
            for rows in (0, c // 2, c // 2 + 3):
                diff, avg = nans(B, c // 2, T), nans(B, c // 2, T)
                cond = nans(B, rows, T) if rows else None
                split(x, mode, diff, avg, cond)
                assert torch.equal(diff.cpu(), want_diff) and torch.equal(avg.cpu(), want_avg), (B, mode, name, rows)
                if rows:
                    assert torch.equal(cond[:, :c // 2].cpu(), want_avg), (B, mode, name, rows)
                    assert bool(torch.isnan(cond[:, c // 2:]).all())
            assert torch.equal(x.cpu(), xc)


@pytest.mark.parametrize("c,T", HAAR)
def test_haar_merge_is_bit_equal(c, T):
    for B, mode in itertools.product([1, 3], [0, 1]):
        a, b = (1.0, 0.5) if mode == 0 else (0.5, 1.0)
        avg, diff = dev("haar/avg%d" % c, (B, c // 2, T)), dev("haar/diff%d" % c, (B, c // 2, T))
        wide = dev("haar/avg2", (B, c // 2 + 2, T))                   # the gradient of a conditioning buffer: only its first rows are read
        for avg2 in (None, wide):
            m = avg.cpu() if avg2 is None else avg.cpu() + avg2[:, :c // 2].cpu()
            want = torch.stack([a * m - b * diff.cpu(), a * m + b * diff.cpu()], 2).reshape(B, c, T)
            for name, out in layouts(B, c, T).items():
                merge(avg, diff, mode, out, avg2)
                assert torch.equal(out.cpu(), want), (B, mode, name)
                if name == "padded":                                  # the elements between the rows were not touched
                    assert bool(torch.isnan(out._base[:, :, c:]).all()) if out._base is not None else True
        # the two kernels invert each other: merge(split(x)) = x up to the roundings of the two
        x = dev("haar/x%d" % c, (B, c, T))
        d2, a2, back = nans(B, c // 2, T), nans(B, c // 2, T), nans(B, c, T)
        split(x, 0, d2, a2, None)
        merge(a2, d2, 0, back)
        assert float((back - x).abs().max()) <= 4 * r64.U32 * float(x.abs().max())


def test_haar_backward_modes_are_the_adjoints_and_repeat():
    """mode 1 of each kernel against autograd through the fp32 definition of the other (bit-equal: the same operations), twice."""
    B, c, T = 3, 8, 33
    x = dev("haar/adj", (B, T, c)).transpose(1, 2)
    gd, ga = dev("haar/gd", (B, c // 2, T)), dev("haar/ga", (B, c // 2, T))
    xc = x.cpu().requires_grad_(True)
    d, a = xc[:, 1::2] - xc[:, ::2], (xc[:, ::2] + xc[:, 1::2]) * 0.5
    (d * gd.cpu()).sum().backward(retain_graph=True)
    g_from_diff = xc.grad.clone()
    xc.grad = None
    (a * ga.cpu()).sum().backward()
    runs = []
    for _ in range(2):
        dx = nans(B, T, c).transpose(1, 2)
        merge(ga, gd, 1, dx)
        runs.append(dx.cpu())
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(runs[0], xc.grad + g_from_diff)                # 0.5 ga -+ gd: one rounding either way
    gz = dev("haar/gz", (B, c, T))
    runs = []
    for _ in range(2):
        dd, da = nans(B, c // 2, T), nans(B, c // 2, T)
        split(gz, 1, dd, da, None)
        runs.append((dd.cpu(), da.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    g = gz.cpu()
    assert torch.equal(runs[0][1], g[:, ::2] + g[:, 1::2]) and torch.equal(runs[0][0], 0.5 * (g[:, 1::2] - g[:, ::2]))


# ---- upsampling ------------------------------------------------------------------------------------------------------------------
UP = [(32, 8, 256), (32, 1, 32), (5, 3, 13), (5, 3, 15), (1, 4, 4), (4, 16, 61), (32, 2, 33),
      (4, 16, 9)]                                                     # ... and one whose trailing frames no column reads


@pytest.mark.parametrize("s,F,T", UP)
def test_upsample_forward_and_backward_vs_float64(s, F, T):
    B = 2
    W = r64.upsample_weights64(s, F, T)
    for n_mels, r0 in itertools.product([1, 7, 80], [0, 4]):
        h = dev("up/h%d" % n_mels, (B, n_mels, F))
        h64 = h.cpu().double().requires_grad_(True)
        want = r64.upsample64(h64, s, T)
        fwd_bound = r64.fma_bound(2, torch.einsum("tf,bmf->bmt", W, h64.detach().abs()))
        rows = r0 + n_mels + 2
        for head in ([None] if r0 == 0 else [None, dev("up/head", (B, r0, T))]):
            out = nans(B, rows, T)
            check(_lib.lib().wg_mr_upsample(engine._p(h), engine._p(head), B, n_mels, F, s, T, engine._p(out), rows, r0,
                                            engine._stream(DEV)), "wg_mr_upsample")
            got = out[:, r0:r0 + n_mels].cpu().double()
            assert bool(((got - want.detach()).abs() <= fwd_bound).all()), (n_mels, r0, float((got - want.detach()).abs().max()))
            assert bool(torch.isnan(out[:, r0 + n_mels:]).all())
            if head is None:
                assert bool(torch.isnan(out[:, :r0]).all())
            else:
                assert torch.equal(out[:, :r0], head)
        if s == 1:
            assert torch.equal(out[:, r0:r0 + n_mels], h[..., :T])     # the identity
        if F == 1:
            assert torch.equal(out[:, r0:r0 + n_mels], h.expand(B, n_mels, T))      # a constant

        dout = dev("up/dout", (B, rows, T))
        g64 = dout[:, r0:r0 + n_mels].cpu().double()
        want_dh, = torch.autograd.grad(want, h64, g64)
        bwd_bound = r64.fma_bound(2 * s, torch.einsum("tf,bmt->bmf", W, g64.abs()))
        runs = []
        for _ in range(2):
            dh = nans(B, n_mels, F)
            check(_lib.lib().wg_mr_upsample_backward(engine._p(dout), rows, r0, B, n_mels, F, s, T, engine._p(dh), engine._stream(DEV)),
                  "wg_mr_upsample_backward")
            runs.append(dh.cpu())
        assert torch.equal(runs[0], runs[1])
        assert bool(((runs[0].double() - want_dh).abs() <= bwd_bound).all()), (n_mels, r0, float((runs[0].double() - want_dh).abs().max()))
        unread = W.sum(0) == 0
        assert bool((runs[0][..., unread] == 0).all())
        assert int(unread.sum()) == (13 if (s, F, T) == (4, 16, 9) else 0)


def test_upsample_from_a_misaligned_buffer():
    """T % 4 == 0 but rows that do not start on 16 bytes: the scalar path, same values"""
    B, n_mels, F, s, T = 2, 7, 8, 4, 32
    h = dev("up/mis", (B, n_mels, F))
    a = nans(B, n_mels, T)
    b = nans(B * n_mels * T + 1)[1:].view(B, n_mels, T)
    for out in (a, b):
        check(_lib.lib().wg_mr_upsample(engine._p(h), None, B, n_mels, F, s, T, engine._p(out), n_mels, 0, engine._stream(DEV)), "wg_mr_upsample")
    assert torch.equal(a, b) and not bool(torch.isnan(a).any())


# ---- pack / unpack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(4, 2, 2), (8, 4, 2, 2)], ids=["shipped", "ragged"])
@pytest.mark.parametrize("T", [1, 13, 257])
def test_pack_and_unpack_are_bit_equal(sizes, T):
    B, n_group = 3, sum(sizes)
    parts = [dev("pack/%d" % i, (B, c, T)) for i, c in enumerate(sizes)]
    want = r64.pack64([p.cpu() for p in parts])
    z = nans(B, T * n_group)
    off = 0
    for p in parts:
        engine.mr_pack(p, n_group, off, z)
        off += p.size(1)
        filled = z.view(B, T, n_group)
        assert not bool(torch.isnan(filled[..., :off]).any()) and bool(torch.isnan(filled[..., off:]).all())
    assert torch.equal(z.cpu(), want)
    off = 0
    for p in parts:
        dst = nans(B, p.size(1), T)
        check(_lib.lib().wg_mr_unpack(engine._p(z), B, p.size(1), T, n_group, off, engine._p(dst), engine._stream(DEV)), "wg_mr_unpack")
        assert torch.equal(dst, p)
        off += p.size(1)
    shifted = nans(B * T * n_group + 1)[1:].view(B, T * n_group)       # a latent off 16-byte alignment
    for i, p in enumerate(parts):
        engine.mr_pack(p, n_group, sum(sizes[:i]), shifted)
    assert torch.equal(shifted, z)
    assert torch.equal(engine.mr_unpack(shifted, n_group, 0, sizes[0]), parts[0])


def test_engine_wrappers_shapes():
    """the wrappers of engine.py allocate what the module expects"""
    x = dev("wrap/x", (2, 33, 8)).transpose(1, 2)
    diff, avg, cond = engine.mr_haar_split(x, 0, 4 + 7)
    assert diff.shape == avg.shape == (2, 4, 33) and cond.shape == (2, 11, 33) and diff.is_contiguous()
    h = dev("wrap/h", (2, 7, 7))
    engine.mr_upsample(h, 5, 33, out=cond, r0=4)
    assert torch.equal(cond[:, :4], avg) and torch.equal(cond[:, 4:], engine.mr_upsample(h, 5, 33))
    y = engine.mr_haar_merge(avg, diff, 0, channels_last=True)
    assert y.shape == (2, 8, 33) and y.transpose(1, 2).is_contiguous()
    assert float((y - x).abs().max()) <= 4 * r64.U32 * float(x.abs().max())
    assert engine.mr_upsample_backward(cond, 4, 7, 7, 5).shape == (2, 7, 7)
