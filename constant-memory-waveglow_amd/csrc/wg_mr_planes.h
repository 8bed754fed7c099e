// MRWaveGlow's plumbing on the engine's planes (wg_mr_forward / wg_mr_inverse, host code in wgflow.hip): the Haar split and merge and the
// linear upsampling of wg_mr.h with the same arithmetic -- every value bit for bit what haar_split_kernel, haar_merge_kernel and up_value
// give -- addressed into padded, haloed planes ([B][Cp][P], data at columns [H, H + T): wg_gemm.h) instead of plain [B, c, T] tensors, so
// that a pass never leaves the planes between its first kernel and its last.  Exact fp32 on the vector ALUs, no atomics, no reduction:
// every WG_PREC_* mode gives the same bits and a second run repeats them.
//
//   plane_split_kernel     rows [0, c) of a plane (or, level 0, the audio [B, N] read as [B, T, c]) -> diff = x1 - x0 into the rows of the
//                          state plane the level's latent leaves from, avg = (x0 + x1) / 2 into rows [0, c / 2) of the level's
//                          conditioning plane and (nullable) into the state rows the next stage works on
//   plane_merge_kernel     (avg, diff) rows of two planes -> z0 = avg - diff / 2, z1 = avg + diff / 2 at rows (2i, 2i + 1) of the next
//                          conditioning plane, or (the last merge) straight into the audio [B, N]
//   plane_upsample_kernel  up_value of every (mel row, column) ONCE, stored into the rows of every plane that is conditioned on the mel
//   plane_copy_kernel      rows of one plane -> rows of another
//
// Lanes walk the columns: 16 bytes per access on whole quads of columns (P, H and every plane base are multiples of 16 floats, so a
// row's column 4 q is 16-byte aligned), scalar accesses on the last, partial quad -- the columns [T, Tt) and the halo are never written,
// they stay zero.  The two audio forms have one thread per (item, column) walk that column's c contiguous samples (16 bytes where c is
// a multiple of 4 and the buffer is aligned) and touch the planes one row at a time, coalesced across the lanes.
#pragma once
#include "wg_small.h"
#include "wg_mr.h"

#define MR_MAX_LEVELS 6          // n_group <= 32 halves into even channel counts at most 4 times: 5 levels
#define MR_MAX_DST (MR_MAX_LEVELS + 1)

namespace mr {

struct PlaneSplitArgs {
    const float *audio;      // level 0: [B][N] read as [B][T][2 half]; nullptr: src
    PRef src;                // rows [0, 2 half) at its ch0
    PRef diff, cond, avg;    // avg.p nullable
    Geo g;
    int half, N;
    int vec;                 // 16-byte accesses allowed (planes: every base aligned; audio: 2 half % 4 == 0, aligned rows)
};

__global__ __launch_bounds__(256) void plane_split_kernel(PlaneSplitArgs p)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const Geo &g = p.g;
    if (p.audio) {                                          // one thread per (item, column), all pairs
        if (gid >= (long long)g.B * g.T) return;
        const int t = (int)(gid % g.T), b = (int)(gid / g.T);
        const float *x = p.audio + (size_t)b * p.N + (size_t)t * 2 * p.half;
        if (p.vec) {                                        // half even: two pairs per float4
            for (int i = 0; i < p.half; i += 2) {
                const float4 q = *(const float4 *)(x + 2 * i);
                const float m0 = 0.5f * (q.x + q.y), m1 = 0.5f * (q.z + q.w);
                *paddr(p.diff, g, b, i, t) = q.y - q.x;
                *paddr(p.diff, g, b, i + 1, t) = q.w - q.z;
                *paddr(p.cond, g, b, i, t) = m0;
                *paddr(p.cond, g, b, i + 1, t) = m1;
                if (p.avg.p) { *paddr(p.avg, g, b, i, t) = m0; *paddr(p.avg, g, b, i + 1, t) = m1; }
            }
            return;
        }
        for (int i = 0; i < p.half; ++i) {
            const float u = x[2 * i], v = x[2 * i + 1];
            const float m = 0.5f * (u + v);
            *paddr(p.diff, g, b, i, t) = v - u;
            *paddr(p.cond, g, b, i, t) = m;
            if (p.avg.p) *paddr(p.avg, g, b, i, t) = m;
        }
        return;
    }
    const long long tq = (g.T + 3) / 4;                     // one thread per (item, pair, 4 columns)
    if (gid >= (long long)g.B * p.half * tq) return;
    const int t0 = (int)(gid % tq) * 4, i = (int)((gid / tq) % p.half), b = (int)(gid / (tq * p.half));
    const float *x0 = paddr(p.src, g, b, 2 * i, t0), *x1 = paddr(p.src, g, b, 2 * i + 1, t0);
    float *d = paddr(p.diff, g, b, i, t0), *c = paddr(p.cond, g, b, i, t0);
    float *a = p.avg.p ? paddr(p.avg, g, b, i, t0) : nullptr;
    if (p.vec && t0 + 4 <= g.T) {
        const float4 u = *(const float4 *)x0, v = *(const float4 *)x1;
        *(float4 *)d = make_float4(v.x - u.x, v.y - u.y, v.z - u.z, v.w - u.w);
        const float4 m = make_float4(0.5f * (u.x + v.x), 0.5f * (u.y + v.y), 0.5f * (u.z + v.z), 0.5f * (u.w + v.w));
        *(float4 *)c = m;
        if (a) *(float4 *)a = m;
        return;
    }
    for (int k = 0; k < 4 && t0 + k < g.T; ++k) {
        const float u = x0[k], v = x1[k];
        const float m = 0.5f * (u + v);
        d[k] = v - u;
        c[k] = m;
        if (a) a[k] = m;
    }
}

struct PlaneMergeArgs {
    PRef avg, diff;          // rows [0, half) at their ch0
    PRef out;                // rows [0, 2 half) at its ch0; out.p == nullptr: audio
    float *audio;            // the last merge: [B][N] written as [B][T][2 half]
    Geo g;
    int half, N;
    int vec;
};

__global__ __launch_bounds__(256) void plane_merge_kernel(PlaneMergeArgs p)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const Geo &g = p.g;
    if (!p.out.p) {                                         // one thread per (item, column), all pairs
        if (gid >= (long long)g.B * g.T) return;
        const int t = (int)(gid % g.T), b = (int)(gid / g.T);
        float *z = p.audio + (size_t)b * p.N + (size_t)t * 2 * p.half;
        if (p.vec) {
            for (int i = 0; i < p.half; i += 2) {
                const float m0 = *paddr(p.avg, g, b, i, t), m1 = *paddr(p.avg, g, b, i + 1, t);
                const float d0 = *paddr(p.diff, g, b, i, t), d1 = *paddr(p.diff, g, b, i + 1, t);
                *(float4 *)(z + 2 * i) = make_float4(m0 - 0.5f * d0, m0 + 0.5f * d0, m1 - 0.5f * d1, m1 + 0.5f * d1);
            }
            return;
        }
        for (int i = 0; i < p.half; ++i) {
            const float m = *paddr(p.avg, g, b, i, t), d = *paddr(p.diff, g, b, i, t);
            z[2 * i] = m - 0.5f * d;
            z[2 * i + 1] = m + 0.5f * d;
        }
        return;
    }
    const long long tq = (g.T + 3) / 4;                     // one thread per (item, pair, 4 columns)
    if (gid >= (long long)g.B * p.half * tq) return;
    const int t0 = (int)(gid % tq) * 4, i = (int)((gid / tq) % p.half), b = (int)(gid / (tq * p.half));
    const float *mp = paddr(p.avg, g, b, i, t0), *dp = paddr(p.diff, g, b, i, t0);
    float *z0 = paddr(p.out, g, b, 2 * i, t0), *z1 = paddr(p.out, g, b, 2 * i + 1, t0);
    if (p.vec && t0 + 4 <= g.T) {
        const float4 m = *(const float4 *)mp, d = *(const float4 *)dp;
        *(float4 *)z0 = make_float4(m.x - 0.5f * d.x, m.y - 0.5f * d.y, m.z - 0.5f * d.z, m.w - 0.5f * d.w);
        *(float4 *)z1 = make_float4(m.x + 0.5f * d.x, m.y + 0.5f * d.y, m.z + 0.5f * d.z, m.w + 0.5f * d.w);
        return;
    }
    for (int k = 0; k < 4 && t0 + k < g.T; ++k) {
        const float m = mp[k], d = dp[k];
        z0[k] = m - 0.5f * d;
        z1[k] = m + 0.5f * d;
    }
}

struct PlaneUpArgs {
    const float *h;          // [B][n_mels][F]
    PRef dst[MR_MAX_DST];    // rows [0, n_mels) at each one's ch0
    Geo g;
    int nd, n_mels, F, s;
    int vec;
};

// one thread per (item, mel row, 4 columns): the values are formed once and stored into every destination
__global__ __launch_bounds__(256) void plane_upsample_kernel(PlaneUpArgs p)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const Geo &g = p.g;
    const long long tq = (g.T + 3) / 4;
    if (gid >= (long long)g.B * p.n_mels * tq) return;
    const int t0 = (int)(gid % tq) * 4, m = (int)((gid / tq) % p.n_mels), b = (int)(gid / (tq * p.n_mels));
    const float *hrow = p.h + ((size_t)b * p.n_mels + m) * p.F;
    if (p.vec && t0 + 4 <= g.T) {
        const float4 v = make_float4(up_value(hrow, t0, p.s, p.F), up_value(hrow, t0 + 1, p.s, p.F), up_value(hrow, t0 + 2, p.s, p.F),
                                     up_value(hrow, t0 + 3, p.s, p.F));
        for (int j = 0; j < p.nd; ++j) *(float4 *)paddr(p.dst[j], g, b, m, t0) = v;
        return;
    }
    for (int k = 0; k < 4 && t0 + k < g.T; ++k) {
        const float v = up_value(hrow, t0 + k, p.s, p.F);
        for (int j = 0; j < p.nd; ++j) paddr(p.dst[j], g, b, m, t0)[k] = v;
    }
}

// one thread per (item, row, 4 columns)
__global__ __launch_bounds__(256) void plane_copy_kernel(PRef src, PRef dst, Geo g, int rows, int vec)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long tq = (g.T + 3) / 4;
    if (gid >= (long long)g.B * rows * tq) return;
    const int t0 = (int)(gid % tq) * 4, r = (int)((gid / tq) % rows), b = (int)(gid / (tq * rows));
    const float *s = paddr(src, g, b, r, t0);
    float *d = paddr(dst, g, b, r, t0);
    if (vec && t0 + 4 <= g.T) { *(float4 *)d = *(const float4 *)s; return; }
    for (int k = 0; k < 4 && t0 + k < g.T; ++k) d[k] = s[k];
}

// logdet[b] = sum_k coef_k log|det W_k| + the partial log_s sums in a fixed order; the sign of T log|det W| is per flow: flows [0, n_a)
// take coef_a, the others coef_b (a reverse_mode model's level 1x1 convs run W^-1 where its prior ones run W)
__global__ void logdet_finalize2_kernel(const float *__restrict__ lu, int ostride, int n_flows, int n_a, float coef_a, float coef_b,
                                        const float *__restrict__ partial, int ntile, int B, float *__restrict__ logdet)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int e = lane; e < n_flows * ntile; e += 64) {
        const int k = e / ntile, i = e - k * ntile;
        s += partial[((size_t)k * B + b) * ntile + i];
    }
    for (int k = lane; k < n_flows; k += 64) s += (k < n_a ? coef_a : coef_b) * lu[(size_t)k * ostride + 2 * WG_MAXC * WG_MAXC];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) logdet[b] = s;
}

}  // namespace mr
