"""Float64 restatements of MelGlow's pieces in plain torch, shared by the CPU and the GPU tests (this directory is on sys.path), the
layer shapes at which the LVC kernels are compared with them, and the float64 side of a wg_mg_gemm product gathered with the
descriptor's own stride formula (include/wgflow.h).  Nothing here launches a kernel or reads the upstream reference."""
import numpy as np
import torch
import torch.nn.functional as Fn

import fill

U32 = 2.0 ** -24      # unit roundoff of fp32

# (R, D, S, radix, L, F, B, dilation, last): every one passes wg_lvc_check; none lands on the kernels' 24 / 16 / 32 steps throughout
LAYER_SHAPES = [
    (12, 10, 6, 5, 25, 5, 3, 1, False),        # R radix = 60 = 24 + 24 + 12; 2D = 20; L = 16 + 9
    (12, 10, 6, 5, 25, 5, 3, 8, False),        # taps cross into the neighbouring frame (two kernels per tile in dX)
    (12, 10, 6, 5, 25, 5, 3, 64, True),        # outer taps leave the signal, inner ones do not
    (12, 10, 6, 5, 25, 5, 3, 128, False),      # dilation > T: only the centre tap is ever inside
    (20, 42, 8, 7, 17, 4, 2, 3, False),        # 2D = 84 = 5 * 16 + 4 = 2 * 32 + 20; R radix = 140
    (16, 16, 16, 3, 128, 2, 1, 32, False),     # D L = R L = 2048 and L = 128: both limits, every per-thread slot in use
    (128, 128, 4, 1, 16, 3, 1, 1, True),       # radix 1, R = D = 128: full LDS arrays, 2D = 256
    (85, 9, 5, 3, 24, 3, 2, 16, False),        # R radix = 255, R L = 2040
    (28, 7, 3, 9, 13, 6, 2, 5, False),         # radix 9, R radix = 252, 2D = 14 < 16
    (6, 5, 4, 3, 1, 9, 2, 2, False),           # one column per frame
    (10, 6, 4, 5, 100, 1, 2, 64, False),       # one frame
]


def shape_id(s):
    return "R%d-D%d-S%d-K%d-L%d-F%d-B%d-d%d-%s" % (s[:8] + ("last" if s[8] else "mid",))


def lvc_inputs(tag, R, D, radix, L, F, B):
    """x [B, R, F L] and predicted kernels [B, F, 2D, R, radix] (numpy float32).  Each (item, frame) kernel carries a scale of its own
    that differs by a factor of 2.5 or more from both neighbouring frames', so a kernel read from the wrong frame is far off."""
    x = fill.normal(tag + "/x", (B, R, F * L))
    w = fill.normal(tag + "/w", (B, F, 2 * D, R, radix), 1.0 / np.sqrt(R * radix))
    scale = np.array([1.0, 2.5, 0.4], np.float32)[(np.arange(B)[:, None] + np.arange(F)[None, :]) % 3]
    return x, w * scale[:, :, None, None, None]


def lvc_conv64(x, w, dilation):
    """z[b, o, c] = sum_{r, k} w[b, c // L, o, r, k] x[b, r, c + (k - K // 2) dilation], zero outside the signal."""
    B, R, T = x.shape
    nf, K = w.shape[1], w.shape[-1]
    L = T // nf
    z = 0
    for k in range(K):
        src = torch.arange(T, device=x.device) + (k - K // 2) * dilation
        ok = ((src >= 0) & (src < T)).to(x.dtype)
        xs = x[:, :, src.clamp(0, T - 1)] * ok
        wk = w[..., k].repeat_interleave(L, dim=1)                    # [B, T, 2D, R]
        z = z + torch.einsum("btor,brt->bot", wk, xs)
    return z


def layer64(x, w, dilation, wo, R, last):
    z = lvc_conv64(x, w, dilation)
    D = z.size(1) // 2
    g = torch.tanh(z[:, :D]) * torch.sigmoid(z[:, D:])
    out = torch.einsum("od,bdt->bot", wo, g)
    return (None, out) if last else (x + out[:, :R], out[:, R:])


def wnorm64(g, v):
    v2 = v.reshape(v.size(0), -1)
    return v2 * (g.reshape(-1, 1) / v2.norm(dim=1, keepdim=True))


def predictor64(pred, y, training):
    """Predictor.forward in float64 with BatchNorm from torch.nn.functional on float64 copies of the buffers."""
    bufs = {}

    def bn(m, a):
        rm, rv = m.running_mean.detach().double().clone(), m.running_var.detach().double().clone()
        out = Fn.batch_norm(a, rm, rv, m.weight.double(), m.bias.double(), training, m.momentum, m.eps)
        bufs[id(m)] = (rm, rv)
        return out

    G = pred.groups
    h = torch.tanh(bn(pred.start[1], Fn.conv1d(y, pred.start[0].weight.double())))
    for blk in pred.res_blocks:
        a = torch.tanh(bn(blk[1], Fn.conv1d(h, blk[0].weight.double(), groups=G)))
        h = torch.tanh(bn(blk[4], Fn.conv1d(a, blk[3].weight.double(), groups=G))) + h
    return Fn.conv1d(h, pred.end.weight.double(), groups=G), bufs


# ---- wg_mg_gemm ------------------------------------------------------------------------------------------------------------------
def gemm_offsets(M, N, K, batch, N1, K1, a, b, c, device="cpu"):
    """Element offsets (int64) of A [batch, M, K], B [batch, K, N] and C [batch, M, N] from their origins, by the formula of
    wg_mg_gemm_desc: n = n2 N1 + n1, k = k2 K1 + k1."""
    ar = lambda n: torch.arange(n, dtype=torch.int64, device=device)
    m, n, k, bt = ar(M), ar(N), ar(K), ar(batch)
    a_m, a_k, a_k2, a_b = a
    b_k, b_k2, b_n, b_n2, b_b = b
    c_m, c_n, c_n2, c_b = c
    ko_a = (k % K1) * a_k + (k // K1) * a_k2
    ko_b = (k % K1) * b_k + (k // K1) * b_k2
    no_b = (n % N1) * b_n + (n // N1) * b_n2
    no_c = (n % N1) * c_n + (n // N1) * c_n2
    ia = bt[:, None, None] * a_b + m[None, :, None] * a_m + ko_a[None, None, :]
    ib = bt[:, None, None] * b_b + ko_b[None, :, None] + no_b[None, None, :]
    ic = bt[:, None, None] * c_b + m[None, :, None] * c_m + no_c[None, None, :]
    return ia, ib, ic


def gemm_expect(A, B, D, offs, alpha, beta, K, splits):
    """(C64, bound) of alpha A B + beta D in float64 from the flat operands (any float dtype) and gemm_offsets' indices.  bound is the
    fp32 fma chain's per-element error: (K + splits + 2) 2^-24 (|alpha| sum_k |a_k b_k| + |beta d|)."""
    ia, ib, ic = offs
    A64, B64 = A.double()[ia], B.double()[ib]
    C64 = alpha * torch.bmm(A64, B64)
    mag = abs(alpha) * torch.bmm(A64.abs(), B64.abs())
    if D is not None:
        D64 = D.double()[ic]
        C64 = C64 + beta * D64
        mag = mag + abs(beta) * D64.abs()
    return C64, (K + splits + 2) * U32 * mag
