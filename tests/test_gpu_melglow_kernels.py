"""The kernels of csrc/wg_lvc.h one by one on the MI355X (-m gpu), at shapes that do not land on their internal steps: wg_mg_gemm
(64 x 64 x 16 tiles, four operand layouts, two-level axes, batches, the split along K and its reduce), the three LVC kernels and the
gate backward, the LVC layer, BatchNorm / weight norm, the predictor.  Every case compares every element of every output with
float64 computed by plain torch on the same inputs (golden/mg_ref64.py).

Bars.  A product or LVC sum of n terms is an fp32 fma chain: |c - c64| <= (n + splits + 2) 2^-24 (|alpha| sum |a b| + |beta d|) per
element, and in addition the 1e-4 of the tensor's max of test_gpu_melglow.py.  What goes through tanhf / expf (not correctly rounded):
1e-5 of max for activations, 1e-4 of max for gradients; BatchNorm statistics 1e-5 of max."""
import ctypes as C

import numpy as np
import pytest
import torch

import fill
import make_golden_melglow as mgg
import mg_ref64 as r64
import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import _lib, engine, melglow as mg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAD_RTOL, STAT_RTOL, ACT_RTOL = 1e-4, 1e-5, 1e-5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def within(what, got, want, bound, rtol=GRAD_RTOL):
    """every element of got within its own bound of want (float64) and within rtol of want's max-abs"""
    got, want, bound = got.double().cpu(), want.double().cpu(), bound.double().cpu()
    assert got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    err = (got - want).abs()
    scale = max(float(want.abs().max()), 1e-30)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max err %.3e (%.3e of max), worst err / bound %.3f" % (what, float(err.max()), float(err.max()) / scale, worst))
    assert bool((err <= bound).all()), "%s: %d elements outside the fma-chain bound, worst %.2f x" % (what, int((err > bound).sum()), worst)
    assert float(err.max()) <= rtol * scale, what


# ---- wg_mg_gemm ------------------------------------------------------------------------------------------------------------------
def roundup16(v):
    return (v + 15) // 16 * 16


def strides(M, N, K, N1, K1, a_kfast, b_kfast, pad):
    """Strides of A, B, C for the two-level axes n = n2 N1 + n1, k = k2 K1 + k1 with `pad` unused elements after every block of every
    level (so a_k2 != K1 a_k and so on), the batch stride larger than the matrix; returns (a, b, c, floats per batch of A, B, C)."""
    nk2, nn2 = (K + K1 - 1) // K1, (N + N1 - 1) // N1
    if a_kfast:                                       # [m][k2][k1]
        a_k, a_k2 = 1, K1 + pad
        a_m = nk2 * a_k2 + pad
        size_a = M * a_m
    else:                                             # [k2][k1][m]
        a_m, a_k = 1, M + pad
        a_k2 = K1 * a_k + pad
        size_a = nk2 * a_k2
    if b_kfast:                                       # [n2][n1][k2][k1]
        b_k, b_k2 = 1, K1 + pad
        b_n = nk2 * b_k2 + pad
        b_n2 = N1 * b_n + pad
        size_b = nn2 * b_n2
    else:                                             # [k2][k1][n2][n1]
        b_n, b_n2 = 1, N1 + pad
        b_k = nn2 * b_n2 + pad
        b_k2 = K1 * b_k + pad
        size_b = nk2 * b_k2
    c_n, c_n2 = 1, N1 + pad                          # [m][n2][n1]
    c_m = nn2 * c_n2 + pad
    size_c = M * c_m
    a_b, b_b, c_b = size_a + 5 + pad, size_b + 3 + pad, size_c + 7 + pad
    return (a_m, a_k, a_k2, a_b), (b_k, b_k2, b_n, b_n2, b_b), (c_m, c_n, c_n2, c_b), (a_b, b_b, c_b)


class Product:
    """One wg_mg_gemm problem on the device: operands whose unused elements are NaN (a read outside the descriptor poisons the
    result), an output whose unused elements must come back untouched."""
    SENTINEL = -777.25

    def __init__(self, tag, M, N, K, batch=1, N1=None, K1=None, a_kfast=True, b_kfast=True, pad=0, layout=None):
        self.M, self.N, self.K, self.batch, self.N1, self.K1 = M, N, K, batch, N1 or N, K1 or K
        if layout is None:
            layout = strides(M, N, K, self.N1, self.K1, a_kfast, b_kfast, pad)
        self.a, self.b, self.c, (na, nb, nc) = layout
        self.offs = r64.gemm_offsets(M, N, K, batch, self.N1, self.K1, self.a, self.b, self.c, DEV)
        ia, ib, ic = self.offs
        for idx, n in zip(self.offs, (na, nb, nc)):
            assert int(idx.max()) < batch * n and int(idx.min()) >= 0
        assert ic.unique().numel() == ic.numel()                                 # no two outputs share an address
        scale = 1.0 / np.sqrt(np.sqrt(K))
        self.A = torch.full((batch * na,), float("nan"), dtype=torch.float32, device=DEV)
        self.B = torch.full((batch * nb,), float("nan"), dtype=torch.float32, device=DEV)
        self.A[ia.reshape(-1)] = dev(fill.normal(tag + "/A", (ia.numel(),), scale))   # (duplicates, e.g. a_m = a_k = 1: last one stays)
        self.B[ib.reshape(-1)] = dev(fill.normal(tag + "/B", (ib.numel(),), scale))
        self.D = torch.full((batch * nc,), float("nan"), dtype=torch.float32, device=DEV)
        self.D[ic.reshape(-1)] = dev(fill.normal(tag + "/D", (ic.numel(),)))
        self.nc = batch * nc
        self.desc = lambda alpha, beta: _lib.WgMgGemmDesc(M, N, K, batch, self.N1, self.K1, *self.a, *self.b, *self.c, alpha, beta)
        self.ws_bytes = int(_lib.lib().wg_mg_gemm_workspace_bytes(C.byref(self.desc(1.0, 1.0))))
        self.splits = self.ws_bytes // (4 * batch * M * N) if self.ws_bytes else 1
        self.kc = roundup16((K + self.splits - 1) // self.splits)

    def run(self, dmode, alpha=1.0, beta=1.0, ws=None, ws_bytes=None):
        """dmode: None (no D), "distinct", "alias" (D is C).  ws None: through engine.mg_gemm; else the library with that workspace."""
        out = torch.full((self.nc,), self.SENTINEL, dtype=torch.float32, device=DEV)
        add = None
        if dmode == "distinct":
            add = self.D
        elif dmode == "alias":
            out.copy_(self.D)
            add = out
        if ws is None:
            engine.mg_gemm(self.A, self.B, out, self.M, self.N, self.K, self.a, self.b, self.c, batch=self.batch, N1=self.N1, K1=self.K1,
                           add=add, alpha=alpha, beta=beta)
        else:
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
            rc = _lib.lib().wg_mg_gemm(C.byref(self.desc(alpha, beta)), p(self.A), p(self.B), p(add), p(out), p(ws),
                                       self.ws_bytes if ws_bytes is None else ws_bytes, engine._stream(DEV))
            assert rc == 0, rc
        torch.cuda.synchronize()
        return out

    def check(self, what, out, dmode, alpha=1.0, beta=1.0):
        want, bound = r64.gemm_expect(self.A, self.B, None if dmode is None else self.D, self.offs, alpha, beta, self.K, self.splits)
        within(what, out[self.offs[2]], want, bound)
        untouched = torch.ones(self.nc, dtype=torch.bool, device=DEV)
        untouched[self.offs[2].reshape(-1)] = False
        before = self.D if dmode == "alias" else torch.full_like(out, self.SENTINEL)
        assert torch.equal(out[untouched].view(torch.int32), before[untouched].view(torch.int32)), "%s: wrote outside C" % what

    def check_all_modes(self, what):
        assert self.ws_bytes == 0 and self.splits == 1, "%s is meant to stay unsplit: choose another shape" % what
        self.check(what + " no D", self.run(None), None)
        self.check(what + " D", self.run("distinct", 0.5, -2.0), "distinct", 0.5, -2.0)
        self.check(what + " D=C", self.run("alias", 0.5, -2.0), "alias", 0.5, -2.0)
        self.check(what + " alpha", self.run(None, -1.75), None, -1.75)


SIZES = [(1, 1, 1), (63, 65, 17), (64, 64, 16), (65, 130, 33), (200, 70, 100)]
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
LAYOUT_IDS = ["Ak-Bk", "Ak-Bn", "Am-Bk", "Am-Bn"]


@pytest.mark.parametrize("a_kfast,b_kfast", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("M,N,K", SIZES)
@pytest.mark.parametrize("batch", [1, 7])
def test_gemm_tile_tails(M, N, K, batch, a_kfast, b_kfast):
    """M, N, K tails of each LDS fill loop; D absent / distinct (alpha 0.5, beta -2) / aliasing C; batch stride > the matrix."""
    p = Product("gemm/t", M, N, K, batch, a_kfast=a_kfast, b_kfast=b_kfast, pad=3)
    if (M, N, K) != (1, 1, 1):                        # (at 1 x 1 x 1 every stride multiplies 0)
        assert (p.a[1] == 1 and p.a[0] != 1) == a_kfast and (p.b[0] == 1 and p.b[2] != 1) == b_kfast     # the loops the case names
    p.check_all_modes("gemm %dx%dx%d b%d" % (M, N, K, batch))


def test_gemm_row_vector_with_unit_strides():
    """M == 1 with a_m == a_k == 1: a row vector times a matrix, A read through the m-fast loop."""
    for K, N in [(33, 70), (100, 5)]:
        a, b, c, sizes = strides(1, N, K, N, K, True, False, 2)
        p = Product("gemm/v", 1, N, K, 3, layout=((1, 1, 0, a[3]), b, c, sizes))
        p.check_all_modes("gemm 1x%dx%d" % (N, K))


@pytest.mark.parametrize("a_kfast,b_kfast", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("M,N,K", SIZES[1:])
@pytest.mark.parametrize("batch", [1, 7])
def test_gemm_two_level_axes(M, N, K, batch, a_kfast, b_kfast):
    """n = n2 N1 + n1 and k = k2 K1 + k1 with padding between the blocks and last blocks that are short."""
    N1, K1 = 11, 7
    if (M, N, K) == (64, 64, 16):
        N1, K1 = 16, 4                                # blocks that divide: the other side of the same arithmetic
    else:
        assert N % N1 and K % K1
    p = Product("gemm/2", M, N, K, batch, N1, K1, a_kfast, b_kfast, pad=2)
    assert p.b[3] != N1 * p.b[2] and p.a[2] != K1 * p.a[1] and p.b[1] != K1 * p.b[0] and p.c[2] != N1 * p.c[1]
    p.check_all_modes("gemm2 %dx%dx%d b%d" % (M, N, K, batch))


class CheckedGemm:
    """engine.mg_gemm, every call of it checked against float64 gathered with the descriptor the caller built"""

    def __init__(self):
        self.real, self.calls = engine.mg_gemm, []

    def __call__(self, A, B, out, M, N, K, a, b, c, batch=1, N1=None, K1=None, add=None, alpha=1.0, beta=1.0):
        flat = lambda t: t.detach().reshape(-1) if t.is_contiguous() else pytest.fail("operand not contiguous")
        d = _lib.WgMgGemmDesc(M, N, K, batch, N1 or N, K1 or K, *a, *b, *c, alpha, beta)
        nbytes = int(_lib.lib().wg_mg_gemm_workspace_bytes(C.byref(d)))
        splits = nbytes // (4 * batch * M * N) if nbytes else 1
        offs = r64.gemm_offsets(M, N, K, batch, N1 or N, K1 or K, a, b, c, DEV)
        for idx, t in zip(offs, (A, B, out)):
            assert int(idx.min()) >= 0 and int(idx.max()) < t.numel()
        want, bound = r64.gemm_expect(flat(A), flat(B), None if add is None else flat(add).clone(), offs, alpha, beta, K, splits)
        res = self.real(A, B, out, M, N, K, a, b, c, batch=batch, N1=N1, K1=K1, add=add, alpha=alpha, beta=beta)
        self.calls.append((M, N, K, batch, N1 or N, K1 or K, splits))
        within("mg_gemm %s" % (self.calls[-1],), flat(out)[offs[2]], want, bound)
        return res


@pytest.mark.parametrize("B,F", [(5, 53), (2, 1)])
def test_gemm_with_the_models_descriptors(B, F, monkeypatch):
    """The descriptors _pred_forward / _pred_backward (both layouts of the predicted kernels), mg_conv1x1, mg_conv1x1_wgrad and the
    grouped products build, at B F = 265 columns and at one frame: each product on its own against float64."""
    chk = CheckedGemm()
    monkeypatch.setattr(engine, "mg_gemm", chk)
    pred = mg.Predictor(7, 50, 5, 2, False, 3)
    pred.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(pred, "kpred/", dict(residual_channels=5, radix=5)).items()})
    pred = pred.to(DEV).train()
    y = dev(fill.normal("kpred/y", (B, 7, F)))
    for reference in (True, False):
        out, ctx = mg._pred_forward(pred, y, reference)
        dy = mg._pred_backward(pred, ctx, dev(fill.normal("kpred/g", tuple(out.shape))), True, {})
        assert dy.shape == y.shape
    n_pred = len(chk.calls)
    assert n_pred == 2 * (2 + 2 * 2 + 4 + 2 * 4)     # forward: start, 2 per block, end; backward: dE, dP, 4 per block, dw0, dy
    T = F * 25
    x, dyv = dev(fill.normal("kpred/x", (B, 10, T))), dev(fill.normal("kpred/dy", (B, 12, T)))
    w = dev(fill.normal("kpred/w", (12, 10), 0.3))
    engine.mg_conv1x1(w, x, add=dyv)
    engine.mg_conv1x1(w, dyv, transpose=True)
    engine.mg_conv1x1(w[3:], dyv[:, 3:].contiguous(), out=x.clone(), add=None, transpose=True)
    engine.mg_conv1x1_wgrad(dyv, x, torch.empty((12, 10), dtype=torch.float32, device=DEV))
    dwo = torch.empty((12, 10), dtype=torch.float32, device=DEV)
    engine.mg_conv1x1_wgrad(dyv[:, :5].contiguous(), x, dwo[:5])
    assert len(chk.calls) == n_pred + 5
    assert all(c[6] == 1 for c in chk.calls[:-2])     # not long enough to be cut ...
    assert all((c[6] > 1) == (B * T >= 1024) and c[5] == T for c in chk.calls[-2:])     # ... but the weight gradients over B T columns


# (M, N, K, batch): 43 exact slices of 512; the shortest K that is cut; a ragged last slice; an empty last slice; several tiles and
# batches; a batch so large that two slices is all that is left
SPLIT_SHAPES = [(48, 48, 22016, 1), (48, 48, 1024, 1), (5, 3, 1031, 1), (48, 48, 32769, 1), (192, 64, 5000, 2), (8, 8, 1024, 200)]
SPLIT_VARIANTS = ["plain", "K1", "D", "D=C"]


def unsplit_product(p):
    """alpha = 1 product of p summed in float64 from mg_gemm calls on dense copies of K < 1024 columns each: none of them is cut"""
    ia, ib, _ = p.offs
    A, B = p.A[ia].contiguous(), p.B[ib].contiguous()                    # [batch, M, K], [batch, K, N]
    total = torch.zeros((p.batch, p.M, p.N), dtype=torch.float64, device=DEV)
    for k0 in range(0, p.K, 1000):
        kn = min(1000, p.K - k0)
        a, b = A[:, :, k0:k0 + kn].contiguous(), B[:, k0:k0 + kn].contiguous()
        d = _lib.WgMgGemmDesc(p.M, p.N, kn, p.batch, p.N, kn, kn, 1, 0, p.M * kn, p.N, 0, 1, 0, kn * p.N, p.N, 1, 0, p.M * p.N, 1.0, 1.0)
        assert _lib.lib().wg_mg_gemm_workspace_bytes(C.byref(d)) == 0
        part = torch.empty((p.batch, p.M, p.N), dtype=torch.float32, device=DEV)
        engine.mg_gemm(a, b, part, p.M, p.N, kn, (kn, 1, 0, p.M * kn), (p.N, 0, 1, 0, kn * p.N), (p.N, 1, 0, p.M * p.N), batch=p.batch)
        total += part.double()
    return total


@pytest.mark.parametrize("variant", SPLIT_VARIANTS)
@pytest.mark.parametrize("M,N,K,batch", SPLIT_SHAPES)
def test_gemm_split_k(M, N, K, batch, variant):
    """The product cut along K: partial slices into a workspace that held NaN, summed by the reduce kernel with alpha / beta / D."""
    K1 = 37 if variant == "K1" else None
    p = Product("gemm/s", M, N, K, batch, K1=K1, a_kfast=True, b_kfast=False, pad=1 if K1 else 0)
    # preconditions (not a specification of gemm_splits: if they fail after a retune, choose other shapes)
    assert p.ws_bytes > 0 and p.splits > 1 and p.ws_bytes == 4 * p.splits * batch * M * N
    assert (p.splits - 1) * p.kc < K or K == 32769
    if K == 32769:
        assert (p.splits - 1) * p.kc >= K             # the last slice starts past K: it must store zeros
    if K in (1031, 5000):
        assert K % p.kc % 16 != 0                     # the last slice is not a whole number of 16-deep steps
    if K1:
        assert p.kc % K1 != 0
    dmode = {"plain": None, "K1": None, "D": "distinct", "D=C": "alias"}[variant]
    alpha, beta = (0.5, -2.0) if dmode else (1.0, 1.0)
    what = "split %dx%dx%d b%d %s (%d slices of %d)" % (M, N, K, batch, variant, p.splits, p.kc)

    nan_ws = lambda extra: torch.full((p.ws_bytes // 4 + extra,), float("nan"), dtype=torch.float32, device=DEV)
    first = p.run(dmode, alpha, beta, ws=nan_ws(0))
    p.check(what, first, dmode, alpha, beta)
    again = p.run(dmode, alpha, beta, ws=nan_ws(0))
    assert torch.equal(first.view(torch.int32), again.view(torch.int32)), what + ": two runs differ"
    roomy = p.run(dmode, alpha, beta, ws=nan_ws(1024), ws_bytes=p.ws_bytes + 4096)
    assert torch.equal(first.view(torch.int32), roomy.view(torch.int32)), what + ": a larger workspace changes the result"
    through_engine = p.run(dmode, alpha, beta)
    assert torch.equal(first.view(torch.int32), through_engine.view(torch.int32)), what

    if dmode is None:                                 # against the same product never cut: a wrong slice boundary is not rounding-size
        want, bound = r64.gemm_expect(p.A, p.B, None, p.offs, 1.0, 1.0, K, p.splits)
        uncut = unsplit_product(p)
        assert bool(((first[p.offs[2]].double() - uncut).abs() <= 2 * bound).all()), what + ": differs from the uncut product"
        assert bool(((uncut - want).abs() <= bound).all())


# ---- the LVC kernels -------------------------------------------------------------------------------------------------------------
def lvc_case(shape):
    R, D, S, radix, L, F, B, dilation, last = shape
    x, w = r64.lvc_inputs("klvc/%d" % dilation, R, D, radix, L, F, B)
    dims = _lib.WgLvcDims(R, D, radix, dilation)
    assert engine.lvc_check(dims, B, F * L, F) == 0
    return dims, dev(x), dev(w)


def chain_bound(n, mag):
    return (n + 2) * r64.U32 * mag


@pytest.mark.parametrize("shape", r64.LAYER_SHAPES, ids=r64.shape_id)
def test_lvc_forward_kernel(shape):
    R, D, S, radix, L, F, B, dilation, last = shape
    dims, x, w = lvc_case(shape)
    z, gate = engine.lvc_forward(dims, x, w, F)
    z64 = r64.lvc_conv64(x.double(), w.double(), dilation)
    mag = r64.lvc_conv64(x.double().abs(), w.double().abs(), dilation)
    within("z", z, z64, chain_bound(R * radix, mag))
    g64 = torch.tanh(z64[:, :D]) * torch.sigmoid(z64[:, D:])
    print("gate: %.3e of max" % rel(gate, g64))
    assert rel(gate, g64) < ACT_RTOL


@pytest.mark.parametrize("shape", r64.LAYER_SHAPES, ids=r64.shape_id)
def test_lvc_backward_kernels(shape):
    """dX (dx_add absent, present, aliasing dx) and dW against float64 autograd of (lvc_conv64(x, w) dz).sum()."""
    R, D, S, radix, L, F, B, dilation, last = shape
    dims, x, w = lvc_case(shape)
    T = F * L
    dz = dev(fill.normal("klvc/dz", (B, 2 * D, T)))
    add = dev(fill.normal("klvc/add", (B, R, T)))

    def grads(xv, wv, dzv):
        xv, wv = xv.double().requires_grad_(True), wv.double().requires_grad_(True)
        (r64.lvc_conv64(xv, wv, dilation) * dzv.double()).sum().backward()
        return xv.grad, wv.grad

    dx64, dw64 = grads(x, w, dz)
    dx_mag, dw_mag = grads(x.abs(), w.abs(), dz.abs())                        # sum |w dz| per dx element, sum |dz x| per dw element

    within("dx", engine.lvc_backward_data(dims, dz, w, F), dx64, chain_bound(2 * D * radix, dx_mag))
    within("dx + add", engine.lvc_backward_data(dims, dz, w, F, dx_add=add), dx64 + add.double(),
           chain_bound(2 * D * radix, dx_mag + add.double().abs()))
    buf = add.clone()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.lib().wg_lvc_backward_data(C.byref(dims), p(dz), p(w), p(buf), B, T, F, p(buf), engine._stream(DEV))
    assert rc == 0
    within("dx += in place", buf, dx64 + add.double(), chain_bound(2 * D * radix, dx_mag + add.double().abs()))

    dw = torch.full_like(w, float("nan"))
    engine.lvc_backward_weight(dims, dz, x, F, dw)
    within("dw", dw, dw64, chain_bound(L, dw_mag))


@pytest.mark.parametrize("B,D,T", [(1, 1, 1), (3, 5, 51), (2, 16, 256), (2, 7, 257)])
def test_lvc_gate_backward_kernel(B, D, T):
    z = dev(fill.normal("kgate/z", (B, 2 * D, T), 1.5))
    dg = dev(fill.normal("kgate/dg", (B, D, T)))
    dz = engine.lvc_gate_backward(z, dg)
    z64 = z.double().requires_grad_(True)
    ((torch.tanh(z64[:, :D]) * torch.sigmoid(z64[:, D:])) * dg.double()).sum().backward()
    print("dz: %.3e of max" % rel(dz, z64.grad))
    assert dz.shape == z.shape and rel(dz, z64.grad) < GRAD_RTOL


@pytest.mark.parametrize("shape", r64.LAYER_SHAPES, ids=r64.shape_id)
def test_lvc_layer_at_ragged_shapes(shape):
    """NonCausalLayerLVC forward + backward as test_gpu_melglow.test_lvc_layer_vs_float64, same bars."""
    R, D, S, radix, L, F, B, dilation, last = shape
    layer = mg.NonCausalLayerLVC(dilation, D, R, S, radix, False, last_layer=last)
    layer.apply(cm.add_weight_norms)
    layer = layer.to(DEV)
    xn, wn = r64.lvc_inputs("klayer/%d" % dilation, R, D, radix, L, F, B)
    x, w = dev(xn).requires_grad_(True), dev(wn).requires_grad_(True)
    res, skip = layer(x, w)
    g_skip = dev(fill.normal("klayer/gs", tuple(skip.shape)))
    loss = (skip * g_skip).sum()
    if not last:
        g_res = dev(fill.normal("klayer/gr", tuple(res.shape)))
        loss = loss + (res * g_res).sum()
    loss.backward()

    x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    g64, v64 = (layer.W_o.weight_g.detach().double().requires_grad_(True), layer.W_o.weight_v.detach().double().requires_grad_(True))
    r, s = r64.layer64(x64, w64, dilation, r64.wnorm64(g64, v64), R, last)
    l64 = (s * g_skip.double()).sum() + (0 if last else (r * g_res.double()).sum())
    l64.backward()
    figures = [("skip", rel(skip, s), 1e-5)] + ([] if last else [("res", rel(res, r), 1e-5)]) + [
        ("dx", rel(x.grad, x64.grad), GRAD_RTOL), ("dw", rel(w.grad, w64.grad), GRAD_RTOL),
        ("dg", rel(layer.W_o.weight_g.grad, g64.grad), GRAD_RTOL), ("dv", rel(layer.W_o.weight_v.grad, v64.grad), GRAD_RTOL)]
    print(" ".join("%s %.2e" % f[:2] for f in figures))
    assert skip.shape == s.shape and x.grad.shape == x.shape and w.grad.shape == w.shape
    for name, err, bar in figures:
        assert err < bar, name


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True], ids=["standard", "mean1000"])
@pytest.mark.parametrize("N", [1, 2, 33, 256, 257, 1000])
@pytest.mark.parametrize("Cn", [1, 5])
def test_batchnorm_kernels(Cn, N, shifted):
    """wg_mg_bn_stats / bn_tanh / bn_tanh_backward / bn_update against the formulas in float64; `shifted`: mean 1000, deviation 1.

    With the mean and 1 / std passed between the launches as fp32 this test measured s off by 1.5e-5 .. 4.3e-5 of max at every
    shifted train case with N >= 2 (x - mean lost the mean's low bits), and dx off by 1.5e-3 .. 4.0e-3 of max at N = 2 in train (the
    backward cancels to order eps there); they are double since (include/wgflow.h), and the worst figure of the file is 1.7e-6."""
    eps = 1e-5
    x = dev(fill.normal("kbn/x%d" % N, (Cn, N)) + (1000.0 if shifted else 0.0))
    rm = dev(fill.uniform("kbn/rm", (Cn,), -0.1, 0.1) + (1000.0 if shifted else 0.0))
    rv = dev(fill.uniform("kbn/rv", (Cn,), 0.8, 1.2))
    gamma, beta = dev(fill.uniform("kbn/g", (Cn,), 0.8, 1.2)), dev(fill.uniform("kbn/b", (Cn,), -0.1, 0.1))
    res, ds = dev(fill.normal("kbn/res", (Cn, N))), dev(fill.normal("kbn/ds", (Cn, N)))
    x64 = x.double()
    figures = []

    def hold(what, got, want, bar):
        figures.append("%s %.2e" % (what, rel(got, want)))
        assert got.shape == want.shape and bool(torch.isfinite(got).all()) and rel(got, want) < bar, what

    for train in (1, 0):
        mean, invstd, var_unb = engine.mg_bn_stats(x, eps, train, rm, rv)
        if train:
            mu64 = x64.mean(1)
            var64 = ((x64 - mu64[:, None]) ** 2).mean(1)
            unb64 = var64 * N / (N - 1) if N > 1 else torch.zeros_like(var64)
            if N == 1:
                assert float(var_unb.abs().max()) == 0.0
        else:
            mu64, var64, unb64 = rm.double(), rv.double(), rv.double()
        is64 = 1.0 / torch.sqrt(var64 + eps)
        tag = "train%d " % train
        hold(tag + "mean", mean, mu64, STAT_RTOL)
        hold(tag + "invstd", invstd, is64, STAT_RTOL)
        if N > 1 or not train:
            hold(tag + "var_unbiased", var_unb, unb64, STAT_RTOL)

        for momentum, counted in ((0.1, True), (1.0, False)):
            rm2, rv2, nbt = rm.clone(), rv.clone(), torch.tensor(3, dtype=torch.int64, device=DEV)
            engine.mg_bn_update(rm2, rv2, nbt if counted else None, mean, var_unb, momentum)
            hold(tag + "running_mean m%g" % momentum, rm2, momentum * mu64 + (1 - momentum) * rm.double(), STAT_RTOL)
            hold(tag + "running_var m%g" % momentum, rv2, momentum * unb64 + (1 - momentum) * rv.double(), STAT_RTOL)
            assert int(nbt) == 3 + int(counted)

        for affine in (True, False):
            g, b = (gamma, beta) if affine else (None, None)
            for with_res in (False, True):
                s, total = engine.mg_bn_tanh(x, mean, invstd, g, b, res=res if with_res else None)
                x64g = x64.clone().requires_grad_(True)
                g64 = gamma.double().requires_grad_(True) if affine else None
                b64 = beta.double().requires_grad_(True) if affine else None
                if train:
                    m = x64g.mean(1, keepdim=True)
                    xh = (x64g - m) / torch.sqrt(((x64g - m) ** 2).mean(1, keepdim=True) + eps)
                else:
                    xh = (x64g - mu64[:, None]) * is64[:, None]
                s64 = torch.tanh(xh * g64[:, None] + b64[:, None] if affine else xh)
                tag2 = tag + ("affine " if affine else "plain ") + ("res " if with_res else "")
                hold(tag2 + "s", s, s64, ACT_RTOL)
                if with_res:
                    hold(tag2 + "sum", total, s64 + res.double(), ACT_RTOL)
                else:
                    assert total is None
                # backward from the kernel's own s and statistics, as the model calls it
                (s64 * ds.double()).sum().backward()
                dgamma = torch.empty_like(gamma) if affine else None
                dbeta = torch.empty_like(beta) if affine else None
                dx = engine.mg_bn_tanh_backward(ds, s, x, mean, invstd, g, train, dgamma, dbeta)
                hold(tag2 + "dx", dx, x64g.grad, GRAD_RTOL)
                if affine:
                    hold(tag2 + "dgamma", dgamma, g64.grad, GRAD_RTOL)
                    hold(tag2 + "dbeta", dbeta, b64.grad, GRAD_RTOL)
    print("\n".join(figures))


# ---- weight norm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 3, 256, 257, 700])
@pytest.mark.parametrize("rows", [1, 7])
def test_weight_norm_kernels(rows, cols):
    v = dev(fill.normal("kwn/v%d" % cols, (rows, cols, 1)))
    g = dev(fill.uniform("kwn/g", (rows, 1, 1), 0.5, 1.5))
    dw = dev(fill.normal("kwn/dw", (rows, cols, 1)))
    w = engine.mg_weight_norm(g, v)
    g64, v64 = g.double().requires_grad_(True), v.double().requires_grad_(True)
    w64 = r64.wnorm64(g64, v64)
    (w64 * dw.double().reshape(rows, cols)).sum().backward()
    assert w.shape == (rows, cols) and rel(w, w64) < ACT_RTOL
    dg, dv = engine.mg_weight_norm_backward(g, v, dw)
    print("w %.2e dg %.2e dv %.2e" % (rel(w, w64), rel(dg, g64.grad), rel(dv, v64.grad)))
    assert dg.shape == g.shape and dv.shape == v.shape
    assert rel(dg, g64.grad) < GRAD_RTOL
    if cols == 1:
        # w = g sign(v): dv = (g / |v|) dw - (g v dw / |v|^3) v is zero in exact arithmetic, and float64 autograd's own answer is its
        # rounding of that difference.  What is left is the rounding of the two equal terms: two factors and two products in fp32.
        assert bool((dv.double().abs() <= 4 * r64.U32 * (g.double() * dw.double() / v.double()).abs()).all())
    else:
        assert rel(dv, v64.grad) < GRAD_RTOL
    dv2 = torch.empty_like(v)                          # dg NULL: the same dv
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.lib().wg_mg_weight_norm_backward(p(g), p(v), p(dw), rows, cols, C.c_void_p(0), p(dv2), engine._stream(DEV))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(dv, dv2)


# ---- the predictor ---------------------------------------------------------------------------------------------------------------
def ragged_predictor(training):
    cfg = (7, 50, 5, 2, False, 3)                       # in, out, hidden, layers, bias, groups
    pred = mg.Predictor(*cfg)
    vals = {k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(pred, "kpred/", dict(residual_channels=5, radix=5)).items()}
    pred.load_state_dict(vals)
    ref = mg.Predictor(*cfg)
    ref.load_state_dict(vals)
    return pred.to(DEV).train(training), ref.double().to(DEV)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,F", [(5, 53), (2, 1), (1, 1)])
def test_predictor_at_ragged_sizes(B, F, training):
    pred, ref = ragged_predictor(training)
    y = dev(fill.normal("kpred/y", (B, 7, F))).requires_grad_(True)
    if training and B * F == 1:
        with pytest.raises(ValueError, match="more than 1 value per channel"):       # as torch's BatchNorm does
            pred(y)
        return
    out = pred(y)
    gout = dev(fill.normal("kpred/g", tuple(out.shape)))
    (out * gout).sum().backward()
    y64 = y.detach().double().requires_grad_(True)
    o64, bufs = r64.predictor64(ref, y64, training)
    (o64 * gout.double()).sum().backward()
    figures = [("out", rel(out, o64), 1e-5), ("dy", rel(y.grad, y64.grad), GRAD_RTOL)]
    figures += [(n, rel(p.grad, p64.grad), GRAD_RTOL) for (n, p), p64 in zip(pred.named_parameters(), ref.parameters())]
    for (n, m), m64 in zip(pred.named_modules(), ref.modules()):
        if isinstance(m, torch.nn.BatchNorm1d):
            rm, rv = bufs[id(m64)]
            figures += [(n + ".running_mean", rel(m.running_mean, rm), STAT_RTOL), (n + ".running_var", rel(m.running_var, rv), STAT_RTOL)]
            assert int(m.num_batches_tracked) == 3 + int(training)
    print("\n".join("%s %.2e" % f[:2] for f in figures))
    assert out.shape == o64.shape == (B, 3 * 50, F)
    for name, err, bar in figures:
        assert err < bar, name
