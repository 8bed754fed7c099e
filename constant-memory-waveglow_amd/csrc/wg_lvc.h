// MelGlow's transform (model/melglow.py upstream): the location-variable convolution (LVC) of WN_LVC and the grouped 1x1 /
// BatchNorm / tanh stack of its kernel predictor.  Exact fp32 on the vector ALUs (fmaf chains, no MFMA), so every
// WG_PREC_* mode gives the same bits here.  Every reduction has a fixed order (LDS trees, no atomics): the recompute of the
// constant-memory backward reproduces the forward bit for bit.
//
//   wg_mg_gemm           C[b] = alpha * A[b] B[b] + beta * D[b] over arbitrary element strides, with the N and K axes
//                        optionally split in two levels (n = n2 * N1 + n1, k = k2 * K1 + k1).  That one kernel covers every
//                        product of the predictor (its [channels, B * frames] activations read straight from a [B, C, F] tensor)
//                        and the 1x1 convs of the WN (batched over items, or summed over items for a weight gradient).
//                        64 x 64 tiles, 16-deep K steps through LDS, 4 x 4 outputs per thread; a product of few tiles and a
//                        long K is cut along K, its partial slices added in slice order by a second launch (gemm_splits).
//   wg_mg_bn_*           BatchNorm1d statistics per channel row (two passes in double, LDS tree; mean and 1 / std stay in double
//                        between the launches: x - mean must not lose the low bits of a large mean, and with two values per
//                        channel the backward is a difference of order eps), the fused normalise + tanh (+ residual), its
//                        backward with batch or running statistics, and the running-stat update on its own.
//   wg_mg_weight_norm*   w = g v / ||v|| per output row and its backward.
//   wg_lvc_forward       one workgroup per (item, frame): z[2D, L] = W_f[2D, R K] . X_unfold[R K, L] with the gate in the
//                        epilogue.  W_f is read exactly once, in 24-column slices staged in LDS (coalesced rows of
//                        the frame's contiguous [2D][R][K] block); the unfolded window is staged next to it.
//   lvc_layer_kernel     a whole NonCausalLayerLVC of an eval pass in one launch: the same K walk, the gate tile kept in LDS, W_o,
//                        residual and skip in the same workgroup (launched from wg_mgflow.h: wg_mg_forward / wg_mg_inverse)
//   wg_lvc_backward_*    dX as a gather (each output column sums its K taps, each tap under the kernel of the frame it came
//                        from: at most two frames per tap and tile, staged in LDS), so overlapping windows add without atomics;
//                        dW_f = dz_f . X_unfold_f^T per (item, frame, 32-row slice).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#define MG_BM 64
#define MG_BN 64
#define MG_BK 16

#define LVC_JC 24         // K slice of the forward (columns of W_f per LDS stage)
#define LVC_MAXD 128      // dilation channels (2 D rows of W_f in LDS)
#define LVC_MAXR 128      // residual channels
#define LVC_MAXRK 256     // R * radix
#define LVC_MAXL 128      // columns per frame
#define LVC_ITEMS 8       // outputs per thread: D * L <= 2048 and R * L <= 2048
#define LVC_OC 16         // output rows of W_f per LDS stage of dX
#define LVC_OR 32         // rows of dW_f per workgroup
#define LVC_TC 16         // columns per LDS stage of dW
#define LVC_WITEMS (LVC_OR * LVC_MAXRK / 256)

namespace mg {

struct GemmArgs {
    wg_mg_gemm_desc d;
    const float *A, *B, *D;
    float *C;
    int splits, kc;      // K cut in `splits` slices of kc (a multiple of MG_BK); splits > 1: raw partials to ws[s][batch][M][N]
    float *ws;
    // gemm_kernel<true> (the eval predictor, wg_mgflow.h): C = tanh(BatchNorm(A B)) (+ bn_res at C's offsets) with the packed running
    // statistics of channel bat * M + m; never with a K cut
    const double *bn_mean, *bn_invstd;
    const float *bn_gamma, *bn_beta, *bn_res;
};

// BatchNorm1d + tanh of one value of channel c from double statistics: the arithmetic of bn_tanh_kernel and of gemm_kernel<true>
__device__ inline float bn_tanh_value(float x, double mean, double invstd, const float *gamma, const float *beta, int c)
{
    float v = (float)(((double)x - mean) * invstd);
    if (gamma) v *= gamma[c];
    if (beta) v += beta[c];
    return tanhf(v);
}

// split-K: how many K slices a product is cut into (1 = none).  Only a product whose tiles leave most of the chip idle and whose
// K is long (the weight gradients: 48 x 48 outputs over 22 016 columns) is cut; each slice is at least 512 deep.
inline int gemm_splits(const wg_mg_gemm_desc &d)
{
    const long long tiles = (long long)((d.M + MG_BM - 1) / MG_BM) * ((d.N + MG_BN - 1) / MG_BN) * d.batch;
    if (tiles >= 256 || d.K < 1024) return 1;
    long long s = std::min<long long>((512 + tiles - 1) / tiles, d.K / 512);
    s = std::min<long long>(s, 64);
    if (s * d.batch > 65535) s = 65535 / d.batch;
    return (int)std::max<long long>(s, 1);
}

template <bool BN = false>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs p)
{
    __shared__ float As[MG_BK][MG_BM + 4];
    __shared__ float Bs[MG_BK][MG_BN + 4];
    const wg_mg_gemm_desc &d = p.d;
    const int tid = threadIdx.x, tm = tid / 16, tn = tid % 16;
    const int m0 = blockIdx.y * MG_BM, n0 = blockIdx.x * MG_BN;
    const int split = blockIdx.z % p.splits;
    const long long bat = blockIdx.z / p.splits;
    const int kbeg = split * p.kc, kend = min(d.K, kbeg + p.kc);
    const float *A = p.A + bat * d.a_b;
    const float *Bm = p.B + bat * d.b_b;
    const bool a_kfast = d.a_k == 1 && d.a_m != 1;       // lanes walk the unit-stride axis of each operand
    const bool b_kfast = d.b_k == 1 && d.b_n != 1;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int k0 = kbeg; k0 < kend; k0 += MG_BK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * 256;
            int mm, kk;
            if (a_kfast) { kk = idx % MG_BK; mm = idx / MG_BK; } else { mm = idx % MG_BM; kk = idx / MG_BM; }
            const int m = m0 + mm, k = k0 + kk;
            float v = 0.f;
            if (m < d.M && k < kend) v = A[(long long)m * d.a_m + (long long)(k % d.K1) * d.a_k + (long long)(k / d.K1) * d.a_k2];
            As[kk][mm] = v;
            int nn;
            if (b_kfast) { kk = idx % MG_BK; nn = idx / MG_BK; } else { nn = idx % MG_BN; kk = idx / MG_BN; }
            const int n = n0 + nn, k2 = k0 + kk;
            float w = 0.f;
            if (n < d.N && k2 < kend)
                w = Bm[(long long)(k2 % d.K1) * d.b_k + (long long)(k2 / d.K1) * d.b_k2 + (long long)(n % d.N1) * d.b_n +
                       (long long)(n / d.N1) * d.b_n2];
            Bs[kk][nn] = w;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MG_BK; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[kk][tm + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tn + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + tm + 16 * i;
        if (m >= d.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tn + 16 * j;
            if (n >= d.N) continue;
            if (p.splits > 1) {
                p.ws[(((long long)split * d.batch + bat) * d.M + m) * d.N + n] = acc[i][j];
                continue;
            }
            const long long off = bat * d.c_b + (long long)m * d.c_m + (long long)(n % d.N1) * d.c_n + (long long)(n / d.N1) * d.c_n2;
            float v = d.alpha * acc[i][j];
            if (p.D) v += d.beta * p.D[off];
            if (BN) {
                const int c = (int)bat * d.M + m;
                v = bn_tanh_value(v, p.bn_mean[c], p.bn_invstd[c], p.bn_gamma, p.bn_beta, c);
                if (p.bn_res) v += p.bn_res[off];
            }
            p.C[off] = v;
        }
    }
}

// the split-K epilogue: partial slices summed in slice order, then alpha / beta / D and the output strides
__global__ __launch_bounds__(256) void gemm_reduce_kernel(GemmArgs p)
{
    const wg_mg_gemm_desc &d = p.d;
    const long long total = (long long)d.batch * d.M * d.N;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float s = 0.f;
    for (int sp = 0; sp < p.splits; ++sp) s += p.ws[(long long)sp * total + i];
    const long long bat = i / ((long long)d.M * d.N), r = i % ((long long)d.M * d.N);
    const int m = (int)(r / d.N), n = (int)(r % d.N);
    const long long off = bat * d.c_b + (long long)m * d.c_m + (long long)(n % d.N1) * d.c_n + (long long)(n / d.N1) * d.c_n2;
    float v = d.alpha * s;
    if (p.D) v += d.beta * p.D[off];
    p.C[off] = v;
}

// 256-lane tree sum in LDS (fixed order)
__device__ inline double block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void bn_stats_kernel(const float *x, int N, float eps, int train, const float *rmean, const float *rvar,
                                                       double *mean, double *invstd, float *var_unb)
{
    __shared__ double red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (!train) {
        if (tid == 0) {
            mean[c] = rmean[c];
            invstd[c] = 1.0 / sqrt((double)rvar[c] + (double)eps);
            var_unb[c] = rvar[c];
        }
        return;
    }
    const float *row = x + (long long)c * N;
    double s = 0.0;
    for (int n = tid; n < N; n += 256) s += row[n];
    const double mu = block_sum(s, red) / N;
    double q = 0.0;
    for (int n = tid; n < N; n += 256) {
        const double e = row[n] - mu;
        q += e * e;
    }
    q = block_sum(q, red);
    if (tid == 0) {
        mean[c] = mu;
        invstd[c] = 1.0 / sqrt(q / N + (double)eps);
        var_unb[c] = N > 1 ? (float)(q / (N - 1)) : 0.f;
    }
}

__global__ __launch_bounds__(256) void bn_update_kernel(float *rmean, float *rvar, int64_t *nbt, const double *mean, const float *var_unb,
                                                        int C, float momentum)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        rmean[c] = momentum * (float)mean[c] + (1.f - momentum) * rmean[c];
        rvar[c] = momentum * var_unb[c] + (1.f - momentum) * rvar[c];
    }
    if (c == 0 && nbt) nbt[0] += 1;
}

__global__ __launch_bounds__(256) void bn_tanh_kernel(const float *x, long long N, long long total, const double *mean, const double *invstd,
                                                      const float *gamma, const float *beta, const float *res, float *s, float *sum)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i / N);
    const float t = bn_tanh_value(x[i], mean[c], invstd[c], gamma, beta, c);
    s[i] = t;
    if (res) sum[i] = t + res[i];
}

__global__ __launch_bounds__(256) void bn_tanh_bwd_kernel(const float *ds, const float *s, const float *x, int N, const double *mean,
                                                          const double *invstd, const float *gamma, int train, float *dx, float *dgamma,
                                                          float *dbeta)
{
    __shared__ double red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const long long o = (long long)c * N;
    const double mu = mean[c], is = invstd[c];
    double sd = 0.0, sdx = 0.0;
    for (int n = tid; n < N; n += 256) {
        const float t = s[o + n];
        const float dyh = ds[o + n] * (1.f - t * t);
        sd += dyh;
        sdx += (double)dyh * (((double)x[o + n] - mu) * is);
    }
    sd = block_sum(sd, red);
    sdx = block_sum(sdx, red);
    if (tid == 0) {
        if (dgamma) dgamma[c] = (float)sdx;
        if (dbeta) dbeta[c] = (float)sd;
    }
    const double k = (gamma ? (double)gamma[c] : 1.0) * is;
    const double md = train ? sd / N : 0.0, mdx = train ? sdx / N : 0.0;
    for (int n = tid; n < N; n += 256) {
        const float t = s[o + n];
        const float dyh = ds[o + n] * (1.f - t * t);
        const double xh = ((double)x[o + n] - mu) * is;
        dx[o + n] = (float)(k * ((double)dyh - md - xh * mdx));
    }
}

__global__ __launch_bounds__(256) void wnorm_kernel(const float *g, const float *v, int cols, float *w)
{
    __shared__ double red[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float *vr = v + (long long)r * cols;
    double ss = 0.0;
    for (int c = tid; c < cols; c += 256) ss += (double)vr[c] * vr[c];
    const float scale = g[r] / (float)sqrt(block_sum(ss, red));
    for (int c = tid; c < cols; c += 256) w[(long long)r * cols + c] = vr[c] * scale;
}

__global__ __launch_bounds__(256) void wnorm_bwd_kernel(const float *g, const float *v, const float *dw, int cols, float *dg, float *dv)
{
    __shared__ double red[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long long o = (long long)r * cols;
    double ss = 0.0, dot = 0.0;
    for (int c = tid; c < cols; c += 256) {
        ss += (double)v[o + c] * v[o + c];
        dot += (double)v[o + c] * dw[o + c];
    }
    ss = block_sum(ss, red);
    dot = block_sum(dot, red);
    const double nrm = sqrt(ss);
    if (tid == 0 && dg) dg[r] = (float)(dot / nrm);
    const float a = (float)(g[r] / nrm), b = (float)(g[r] * dot / (nrm * nrm * nrm));
    for (int c = tid; c < cols; c += 256) dv[o + c] = a * dw[o + c] - b * v[o + c];
}

__device__ inline float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(256) void gate_bwd_kernel(const float *z, const float *dg, long long DT, long long T, long long total, float *dz)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / DT, r = i % DT;
    const long long zw = b * 2 * DT + r, zv = zw + DT;
    const float th = tanhf(z[zw]), sg = sigmoidf_(z[zv]), g = dg[i];
    dz[zw] = g * sg * (1.f - th * th);
    dz[zv] = g * th * sg * (1.f - sg);
    (void)T;
}

struct LvcArgs {
    int R, D, K, dil, L, T, F;
};

// The K walk of the forward for frame f of one item: W_f in LVC_JC-column slices and the unfolded window next to it, both staged in LDS;
// thread tid accumulates the two gate rows (c, c + D) of its items tid + 256 i = c L + t.
//   z[b][o][fL + t] = sum_j W_{b,f}[o][j] X_unfold[j][t], j = ci K + k, X_unfold[j][t] = x[b][ci][fL + t + (k - K/2) dil]
__device__ __forceinline__ void lvc_walk(const LvcArgs &a, const float *xb, const float *Wf, int f, float (*Ws)[LVC_JC + 1],
                                         float (*Xs)[LVC_MAXL], float (&aw)[LVC_ITEMS], float (&av)[LVC_ITEMS])
{
    const int tid = threadIdx.x;
    const int RK = a.R * a.K, D2 = 2 * a.D, half = (a.K - 1) / 2, nitems = a.D * a.L;
#pragma unroll
    for (int i = 0; i < LVC_ITEMS; ++i) aw[i] = av[i] = 0.f;
    for (int j0 = 0; j0 < RK; j0 += LVC_JC) {
        const int jn = min(LVC_JC, RK - j0);
        __syncthreads();
        for (int idx = tid; idx < D2 * LVC_JC; idx += 256) {
            const int o = idx / LVC_JC, jj = idx % LVC_JC;
            Ws[o][jj] = jj < jn ? Wf[(long long)o * RK + j0 + jj] : 0.f;
        }
        for (int idx = tid; idx < LVC_JC * a.L; idx += 256) {
            const int jj = idx / a.L, t = idx % a.L;
            float v = 0.f;
            if (jj < jn) {
                const int j = j0 + jj, ci = j / a.K, k = j % a.K;
                const int col = f * a.L + t + (k - half) * a.dil;
                if (col >= 0 && col < a.T) v = xb[(long long)ci * a.T + col];
            }
            Xs[jj][t] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < LVC_ITEMS; ++i) {
            const int item = tid + i * 256;
            if (item < nitems) {
                const int c = item / a.L, t = item % a.L;
                float sw = aw[i], sv = av[i];
                for (int jj = 0; jj < jn; ++jj) {
                    const float xv = Xs[jj][t];
                    sw = fmaf(Ws[c][jj], xv, sw);
                    sv = fmaf(Ws[c + a.D][jj], xv, sv);
                }
                aw[i] = sw;
                av[i] = sv;
            }
        }
    }
}

// forward: grid (F, B); z and the gate of frame f of item b
__global__ __launch_bounds__(256) void lvc_fwd_kernel(LvcArgs a, const float *x, const float *W, float *z, float *gate)
{
    __shared__ float Ws[2 * LVC_MAXD][LVC_JC + 1];
    __shared__ float Xs[LVC_JC][LVC_MAXL];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int D2 = 2 * a.D, nitems = a.D * a.L;
    float aw[LVC_ITEMS], av[LVC_ITEMS];
    lvc_walk(a, x + (long long)b * a.R * a.T, W + ((long long)b * a.F + f) * ((long long)D2 * a.R * a.K), f, Ws, Xs, aw, av);
#pragma unroll
    for (int i = 0; i < LVC_ITEMS; ++i) {
        const int item = tid + i * 256;
        if (item < nitems) {
            const int c = item / a.L, t = item % a.L;
            const long long col = (long long)f * a.L + t;
            z[((long long)b * D2 + c) * a.T + col] = aw[i];
            z[((long long)b * D2 + c + a.D) * a.T + col] = av[i];
            gate[((long long)b * a.D + c) * a.T + col] = tanhf(aw[i]) * sigmoidf_(av[i]);
        }
    }
}

// One NonCausalLayerLVC of an eval pass in one launch (wg_mg_forward / wg_mg_inverse): grid (F, B) as lvc_fwd_kernel and the same K
// walk; the frame's gate tile [D][L] stays in LDS, W_o . gate runs in the same workgroup, and neither z nor the gate reaches memory.
//   hn[b][r][fL + t]   = h[b][r][fL + t] + sum_d wo[r][d] gate[d][t]            (r < R; absent in the last layer)
//   skip[b][s][fL + t] (+)= sum_d wo[R + s][d] gate[d][t]                       (the first layer stores, later layers add in place)
// hn is the OTHER of two planes: the neighbouring frames' workgroups still read this frame's columns of h as their halo.  The
// workgroup owns its L columns of hn and skip.  After the walk its two LDS arrays are free: the gate tile takes the window's
// (D L <= 2048 floats of its 3072) and W_o is staged in the kernel slices' (LVC_WO_FLOATS / D rows at a time), so the launch needs
// no more LDS than lvc_fwd_kernel and four workgroups share a CU.
struct LvcLayerArgs {
    LvcArgs a;
    int S, first, last;
    const float *h, *W, *wo;
    float *hn, *skip;
};
#define LVC_WO_FLOATS (2 * LVC_MAXD * (LVC_JC + 1))

__global__ __launch_bounds__(256) void lvc_layer_kernel(LvcLayerArgs p)
{
    __shared__ float Ws[2 * LVC_MAXD][LVC_JC + 1];
    __shared__ float Xs[LVC_JC][LVC_MAXL];
    static_assert(LVC_JC * LVC_MAXL >= 256 * LVC_ITEMS, "the gate tile must fit the window's array");
    const LvcArgs &a = p.a;
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nitems = a.D * a.L;
    float aw[LVC_ITEMS], av[LVC_ITEMS];
    lvc_walk(a, p.h + (long long)b * a.R * a.T, p.W + ((long long)b * a.F + f) * ((long long)2 * a.D * a.R * a.K), f, Ws, Xs, aw, av);
    float *Gs = &Xs[0][0], *Wo = &Ws[0][0];
    __syncthreads();                                                             // the last slice has been read by everyone
#pragma unroll
    for (int i = 0; i < LVC_ITEMS; ++i) {
        const int item = tid + i * 256;
        if (item < nitems) Gs[item] = tanhf(aw[i]) * sigmoidf_(av[i]);          // Gs[c L + t]
    }
    const int nres = p.last ? 0 : a.R, nrows = nres + p.S, chunk = LVC_WO_FLOATS / a.D;
    for (int r0 = 0; r0 < nrows; r0 += chunk) {
        const int rn = min(chunk, nrows - r0);
        __syncthreads();                                                         // the gate tile is written; the previous rows are used up
        for (int idx = tid; idx < rn * a.D; idx += 256) Wo[idx] = p.wo[(long long)r0 * a.D + idx];
        __syncthreads();
        // four outputs per thread at a time: four independent fma chains (each over d ascending) hide the LDS latency
        for (int item0 = tid; item0 < rn * a.L; item0 += 4 * 256) {
            int wrow[4], t[4];
            float s[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int item = min(item0 + q * 256, rn * a.L - 1);             // (a slot past the end recomputes the last output, unused)
                wrow[q] = item / a.L * a.D;
                t[q] = item % a.L;
                s[q] = 0.f;
            }
            for (int d = 0; d < a.D; ++d) {
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] = fmaf(Wo[wrow[q] + d], Gs[d * a.L + t[q]], s[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int item = item0 + q * 256;
                if (item >= rn * a.L) break;
                const int r = r0 + item / a.L;
                const long long col = (long long)f * a.L + t[q];
                if (r < nres) {
                    const long long off = ((long long)b * a.R + r) * a.T + col;
                    p.hn[off] = s[q] + p.h[off];
                } else {
                    const long long off = ((long long)b * p.S + (r - nres)) * a.T + col;
                    p.skip[off] = p.first ? s[q] : s[q] + p.skip[off];
                }
            }
        }
    }
}

__device__ inline int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// dX: grid (F, B); dx[b][ci][fL + t] = dx_add + sum_k sum_o W_{b, frame(u)}[o][ci][k] dz[b][o][u], u = fL + t - (k - K/2) dil
__global__ __launch_bounds__(256) void lvc_dx_kernel(LvcArgs a, const float *dz, const float *W, const float *dx_add, float *dx)
{
    __shared__ float Ws[2][LVC_OC][LVC_MAXR + 1];
    __shared__ float Ds[LVC_OC][LVC_MAXL];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int RK = a.R * a.K, D2 = 2 * a.D, half = (a.K - 1) / 2, nitems = a.R * a.L;
    const long long wframe = (long long)D2 * RK;
    float acc[LVC_ITEMS];
#pragma unroll
    for (int i = 0; i < LVC_ITEMS; ++i) acc[i] = 0.f;
    for (int k = 0; k < a.K; ++k) {
        const int u0 = f * a.L - (k - half) * a.dil;     // the dz column output column fL reads through tap k
        const int fa = floordiv(u0, a.L);               // its frame; the tile's last column is in fa or fa + 1
        for (int o0 = 0; o0 < D2; o0 += LVC_OC) {
            const int on = min(LVC_OC, D2 - o0);
            __syncthreads();
            for (int idx = tid; idx < 2 * LVC_OC * a.R; idx += 256) {
                const int sel = idx / (LVC_OC * a.R), rem = idx % (LVC_OC * a.R), oo = rem / a.R, ci = rem % a.R;
                const int fr = fa + sel;
                float v = 0.f;
                if (oo < on && fr >= 0 && fr < a.F) v = W[((long long)b * a.F + fr) * wframe + (long long)(o0 + oo) * RK + ci * a.K + k];
                Ws[sel][oo][ci] = v;
            }
            for (int idx = tid; idx < LVC_OC * a.L; idx += 256) {
                const int oo = idx / a.L, t = idx % a.L, u = u0 + t;
                float v = 0.f;
                if (oo < on && u >= 0 && u < a.T) v = dz[((long long)b * D2 + o0 + oo) * a.T + u];
                Ds[oo][t] = v;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < LVC_ITEMS; ++i) {
                const int item = tid + i * 256;
                if (item < nitems) {
                    const int ci = item / a.L, t = item % a.L;
                    const int sel = floordiv(u0 + t, a.L) - fa;
                    float s = acc[i];
                    for (int oo = 0; oo < on; ++oo) s = fmaf(Ws[sel][oo][ci], Ds[oo][t], s);
                    acc[i] = s;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < LVC_ITEMS; ++i) {
        const int item = tid + i * 256;
        if (item < nitems) {
            const int ci = item / a.L, t = item % a.L;
            const long long off = ((long long)b * a.R + ci) * a.T + (long long)f * a.L + t;
            dx[off] = acc[i] + (dx_add ? dx_add[off] : 0.f);
        }
    }
}

// dW: grid (F, B, ceil(2D / 32)); dW_{b,f}[o][j] = sum_t dz[b][o][fL + t] X_unfold[j][t]
__global__ __launch_bounds__(256) void lvc_dw_kernel(LvcArgs a, const float *dz, const float *x, float *dW)
{
    __shared__ float Zs[LVC_OR][LVC_TC + 1];
    __shared__ float Xs[LVC_TC][LVC_MAXRK];
    const int f = blockIdx.x, b = blockIdx.y, o0 = blockIdx.z * LVC_OR, tid = threadIdx.x;
    const int RK = a.R * a.K, D2 = 2 * a.D, half = (a.K - 1) / 2;
    const int on = min(LVC_OR, D2 - o0), nitems = on * RK;
    const float *xb = x + (long long)b * a.R * a.T;
    float acc[LVC_WITEMS];
#pragma unroll
    for (int i = 0; i < LVC_WITEMS; ++i) acc[i] = 0.f;
    for (int t0 = 0; t0 < a.L; t0 += LVC_TC) {
        const int tn = min(LVC_TC, a.L - t0);
        __syncthreads();
        for (int idx = tid; idx < LVC_OR * LVC_TC; idx += 256) {
            const int oo = idx / LVC_TC, tt = idx % LVC_TC;
            Zs[oo][tt] = (oo < on && tt < tn) ? dz[((long long)b * D2 + o0 + oo) * a.T + (long long)f * a.L + t0 + tt] : 0.f;
        }
        for (int idx = tid; idx < LVC_TC * RK; idx += 256) {
            const int tt = idx / RK, j = idx % RK, ci = j / a.K, k = j % a.K;
            const int col = f * a.L + t0 + tt + (k - half) * a.dil;
            Xs[tt][j] = (tt < tn && col >= 0 && col < a.T) ? xb[(long long)ci * a.T + col] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < LVC_WITEMS; ++i) {
            const int item = tid + i * 256;
            if (item < nitems) {
                const int oo = item / RK, j = item % RK;
                float s = acc[i];
#pragma unroll
                for (int tt = 0; tt < LVC_TC; ++tt) s = fmaf(Zs[oo][tt], Xs[tt][j], s);
                acc[i] = s;
            }
        }
    }
    float *out = dW + ((long long)b * a.F + f) * ((long long)D2 * RK) + (long long)o0 * RK;
#pragma unroll
    for (int i = 0; i < LVC_WITEMS; ++i) {
        const int item = tid + i * 256;
        if (item < nitems) out[item] = acc[i];
    }
}

inline int launched() { return hipGetLastError() == hipSuccess ? WG_OK : WG_ELAUNCH; }

}  // namespace mg

extern "C" {

size_t wg_mg_gemm_workspace_bytes(const wg_mg_gemm_desc *d)
{
    if (!d || d->M < 1 || d->N < 1 || d->K < 1 || d->batch < 1) return 0;
    const int s = mg::gemm_splits(*d);
    return s > 1 ? (size_t)s * d->batch * d->M * d->N * sizeof(float) : 0;
}

int wg_mg_gemm(const wg_mg_gemm_desc *d, const float *A, const float *B, const float *D, float *C, void *ws, size_t ws_bytes, void *stream)
{
    if (!d || !A || !B || !C) return WG_EINVAL;
    if (d->M < 1 || d->N < 1 || d->K < 1 || d->batch < 1 || d->N1 < 1 || d->K1 < 1) return WG_EINVAL;
    const long long gy = (d->M + MG_BM - 1) / MG_BM, gx = (d->N + MG_BN - 1) / MG_BN;
    if (gy > 65535 || d->batch > 65535 || gx > 0x7fffffffLL) return WG_EUNSUPPORTED;
    mg::GemmArgs p;
    p.d = *d; p.A = A; p.B = B; p.D = D; p.C = C;
    p.bn_mean = p.bn_invstd = nullptr; p.bn_gamma = p.bn_beta = p.bn_res = nullptr;
    p.splits = mg::gemm_splits(*d);
    p.kc = (d->K + p.splits - 1) / p.splits;
    p.kc = (p.kc + MG_BK - 1) / MG_BK * MG_BK;
    p.ws = (float *)ws;
    if (p.splits > 1 && (!ws || ws_bytes < wg_mg_gemm_workspace_bytes(d))) return WG_EWORKSPACE;
    hipLaunchKernelGGL(mg::gemm_kernel<false>, dim3((unsigned)gx, (unsigned)gy, (unsigned)(d->batch * p.splits)), dim3(256), 0,
                       (hipStream_t)stream, p);
    if (p.splits > 1) {
        if (hipGetLastError() != hipSuccess) return WG_ELAUNCH;
        const long long total = (long long)d->batch * d->M * d->N;
        hipLaunchKernelGGL(mg::gemm_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    }
    return mg::launched();
}

int wg_mg_bn_stats(const float *x, int C, int N, float eps, int train, const float *running_mean, const float *running_var, double *mean,
                   double *invstd, float *var_unbiased, void *stream)
{
    if (C < 1 || N < 1 || !mean || !invstd || !var_unbiased) return WG_EINVAL;
    if (train ? !x : (!running_mean || !running_var)) return WG_EINVAL;
    hipLaunchKernelGGL(mg::bn_stats_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, x, N, eps, train, running_mean, running_var, mean,
                       invstd, var_unbiased);
    return mg::launched();
}

int wg_mg_bn_update(float *running_mean, float *running_var, int64_t *num_batches_tracked, const double *mean, const float *var_unbiased,
                    int C, float momentum, void *stream)
{
    if (C < 1 || !running_mean || !running_var || !mean || !var_unbiased) return WG_EINVAL;
    hipLaunchKernelGGL(mg::bn_update_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, running_mean, running_var,
                       num_batches_tracked, mean, var_unbiased, C, momentum);
    return mg::launched();
}

int wg_mg_bn_tanh(const float *x, int C, int N, const double *mean, const double *invstd, const float *gamma, const float *beta,
                  const float *res, float *s, float *sum, void *stream)
{
    if (!x || C < 1 || N < 1 || !mean || !invstd || !s || (res && !sum)) return WG_EINVAL;
    const long long total = (long long)C * N;
    hipLaunchKernelGGL(mg::bn_tanh_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long long)N, total,
                       mean, invstd, gamma, beta, res, s, sum);
    return mg::launched();
}

int wg_mg_bn_tanh_backward(const float *ds, const float *s, const float *x, int C, int N, const double *mean, const double *invstd,
                           const float *gamma, int train, float *dx, float *dgamma, float *dbeta, void *stream)
{
    if (!ds || !s || !x || C < 1 || N < 1 || !mean || !invstd || !dx) return WG_EINVAL;
    hipLaunchKernelGGL(mg::bn_tanh_bwd_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, ds, s, x, N, mean, invstd, gamma, train, dx,
                       dgamma, dbeta);
    return mg::launched();
}

int wg_mg_weight_norm(const float *g, const float *v, int rows, int cols, float *w, void *stream)
{
    if (!g || !v || !w || rows < 1 || cols < 1) return WG_EINVAL;
    hipLaunchKernelGGL(mg::wnorm_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, g, v, cols, w);
    return mg::launched();
}

int wg_mg_weight_norm_backward(const float *g, const float *v, const float *dw, int rows, int cols, float *dg, float *dv, void *stream)
{
    if (!g || !v || !dw || !dv || rows < 1 || cols < 1) return WG_EINVAL;
    hipLaunchKernelGGL(mg::wnorm_bwd_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, g, v, dw, cols, dg, dv);
    return mg::launched();
}

int wg_lvc_check(const wg_lvc_dims *d, int B, int T, int F)
{
    if (!d || B < 1 || T < 1 || F < 1) return WG_EINVAL;
    if (d->res_ch < 1 || d->dil_ch < 1 || d->radix < 1 || d->dilation < 1) return WG_EINVAL;
    if (!(d->radix & 1)) return WG_EUNSUPPORTED;                     // an even kernel changes the window length upstream
    if (T % F) return WG_ESHAPE;                                      // every frame owns T / F columns
    const int L = T / F;
    if (d->dil_ch > LVC_MAXD || d->res_ch > LVC_MAXR || d->res_ch * d->radix > LVC_MAXRK || L > LVC_MAXL) return WG_EUNSUPPORTED;
    if (d->dil_ch * L > 256 * LVC_ITEMS || d->res_ch * L > 256 * LVC_ITEMS) return WG_EUNSUPPORTED;
    if (B > 65535) return WG_EUNSUPPORTED;
    if ((long long)d->dilation * (d->radix / 2) > (1LL << 30)) return WG_EUNSUPPORTED;
    return WG_OK;
}

static mg::LvcArgs lvc_args(const wg_lvc_dims *d, int T, int F)
{
    mg::LvcArgs a;
    a.R = d->res_ch; a.D = d->dil_ch; a.K = d->radix; a.dil = d->dilation; a.L = T / F; a.T = T; a.F = F;
    return a;
}

int wg_lvc_forward(const wg_lvc_dims *d, const float *x, const float *w, int B, int T, int F, float *z, float *gate, void *stream)
{
    int rc = wg_lvc_check(d, B, T, F);
    if (rc) return rc;
    if (!x || !w || !z || !gate) return WG_EINVAL;
    hipLaunchKernelGGL(mg::lvc_fwd_kernel, dim3(F, B), dim3(256), 0, (hipStream_t)stream, lvc_args(d, T, F), x, w, z, gate);
    return mg::launched();
}

int wg_lvc_backward_data(const wg_lvc_dims *d, const float *dz, const float *w, const float *dx_add, int B, int T, int F, float *dx,
                         void *stream)
{
    int rc = wg_lvc_check(d, B, T, F);
    if (rc) return rc;
    if (!dz || !w || !dx) return WG_EINVAL;
    hipLaunchKernelGGL(mg::lvc_dx_kernel, dim3(F, B), dim3(256), 0, (hipStream_t)stream, lvc_args(d, T, F), dz, w, dx_add, dx);
    return mg::launched();
}

int wg_lvc_backward_weight(const wg_lvc_dims *d, const float *dz, const float *x, int B, int T, int F, float *dw, void *stream)
{
    int rc = wg_lvc_check(d, B, T, F);
    if (rc) return rc;
    if (!dz || !x || !dw) return WG_EINVAL;
    const int gz = (2 * d->dil_ch + LVC_OR - 1) / LVC_OR;
    hipLaunchKernelGGL(mg::lvc_dw_kernel, dim3(F, B, gz), dim3(256), 0, (hipStream_t)stream, lvc_args(d, T, F), dz, x, dw);
    return mg::launched();
}

int wg_lvc_gate_backward(const float *z, const float *dgate, int B, int D, int T, float *dz, void *stream)
{
    if (!z || !dgate || !dz || B < 1 || D < 1 || T < 1) return WG_EINVAL;
    const long long total = (long long)B * D * T;
    hipLaunchKernelGGL(mg::gate_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, dgate,
                       (long long)D * T, (long long)T, total, dz);
    return mg::launched();
}

}  // extern "C"
