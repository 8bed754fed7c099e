// MRWaveGlow's multi-resolution plumbing (model/mr_waveglow.py upstream): everything around its couplings.  Exact fp32 on the vector
// ALUs, no MFMA, no atomics, no reduction across threads: every WG_PREC_* mode gives the same bits and a second run repeats them.
// Split, merge, upsample, pack and unpack are memory-bound streams: lanes walk the unit-stride axis of the side with more traffic, 16-byte
// loads and stores where the shape and the addresses allow (T a multiple of 4 and aligned rows, or whole float4s of channels), scalar
// accesses otherwise.  The upsampling's backward is a gather and no such stream: its lanes run along the frames, so neighbouring lanes
// read columns s apart (each lane walks 3s + 1 consecutive columns, so the lines it touches are reused from cache), and every thread
// recomputes the source pair of each column it visits.  It handles B n_mels F outputs (121 k at the shipped size).
//
//   wg_mr_haar_split     x [B, c, T] by element strides -> diff = a (x1 - x0), avg = b (x0 + x1) over the channel pairs (2i, 2i + 1);
//                        (a, b) = (1, 1/2) is the forward of a level, (1/2, 1) the backward of the merge.  avg may be written a second
//                        time into rows [0, c/2) of a conditioning buffer.  Each output is one rounding of exact operands.
//   wg_mr_haar_merge     (avg, diff) -> z0 = a avg - b diff, z1 = a avg + b diff at channels (2i, 2i + 1) of an output given by element
//                        strides; (a, b) = (1, 1/2) is the merge of the reverse pass, (1/2, 1) the backward of the split.  A second
//                        avg operand (rows of a conditioning buffer's gradient) is added to the first one before anything else.
//   wg_mr_upsample       F.interpolate(h, scale_factor = s, mode = 'linear') cut to T columns, written into rows [r0, r0 + n_mels) of a
//                        wider buffer; rows [0, r0) can be copied from a second tensor in the same launch (cat([x, y], 1)).  The
//                        source position of column t is (2t + 1 - s) / (2s), formed from integers.
//   wg_mr_upsample_backward   the transpose as a gather: one thread per frame sums the columns that read it, in column order.
//   wg_mr_pack / unpack  [B, c, T] <-> channels [off, off + c) of the [B, T, n_group] latent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mr {

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline int launched() { return hipGetLastError() == hipSuccess ? WG_OK : WG_ELAUNCH; }
// blocks of 256 threads for `total` work items; 0 when a grid cannot hold them
inline unsigned blocks_for(long long total) { return total > 0x7fffffffLL * 256 ? 0u : (unsigned)((total + 255) / 256); }

struct HaarArgs {
    const float *x;          // split: the input by strides.  merge: unused
    const float *avg2;       // merge: second avg operand [B, avg2_rows, T] (nullable)
    float *diff, *avg;       // [B, c/2, T]: outputs of the split, inputs of the merge
    float *cond;             // split: second copy of avg, rows [0, c/2) of [B, cond_rows, T] (nullable)
    float *out;              // merge: the output by strides
    long long s_b, s_c, s_t; // element strides of x (split) or out (merge)
    long long rows2;         // cond_rows (split) or avg2_rows (merge)
    int B, half, T;          // half = c / 2
    float a, b;
    int by_column;           // 1: one thread per (item, column) walks the channels (channels are the unit-stride axis of x / out)
    int vec;                 // 16-byte accesses allowed
};

// by_column = 0: one thread per (item, pair, 4 columns); by_column = 1: one thread per (item, column), all pairs.
__global__ __launch_bounds__(256) void haar_split_kernel(HaarArgs p)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long T = p.T, plane = (long long)p.half * T;
    if (!p.by_column) {
        const long long tq = (T + 3) / 4;
        if (gid >= (long long)p.B * p.half * tq) return;
        const long long t0 = (gid % tq) * 4, i = (gid / tq) % p.half, b = gid / (tq * p.half);
        const float *x0 = p.x + b * p.s_b + 2 * i * p.s_c + t0 * p.s_t, *x1 = x0 + p.s_c;
        const long long o = b * plane + i * T + t0;
        float *cond = p.cond ? p.cond + b * p.rows2 * T + i * T + t0 : nullptr;
        if (p.vec) {
            const float4 u = *(const float4 *)x0, v = *(const float4 *)x1;
            *(float4 *)(p.diff + o) = make_float4(p.a * (v.x - u.x), p.a * (v.y - u.y), p.a * (v.z - u.z), p.a * (v.w - u.w));
            const float4 m = make_float4(p.b * (u.x + v.x), p.b * (u.y + v.y), p.b * (u.z + v.z), p.b * (u.w + v.w));
            *(float4 *)(p.avg + o) = m;
            if (cond) *(float4 *)cond = m;
            return;
        }
        for (int k = 0; k < 4 && t0 + k < T; ++k) {
            const float u = x0[k * p.s_t], v = x1[k * p.s_t];
            const float m = p.b * (u + v);
            p.diff[o + k] = p.a * (v - u);
            p.avg[o + k] = m;
            if (cond) cond[k] = m;
        }
        return;
    }
    if (gid >= (long long)p.B * T) return;
    const long long t = gid % T, b = gid / T;
    const float *x = p.x + b * p.s_b + t * p.s_t;
    const long long o = b * plane + t;
    float *cond = p.cond ? p.cond + b * p.rows2 * T + t : nullptr;
    if (p.vec) {                                        // s_c == 1, half even: two pairs per float4
        for (int i = 0; i < p.half; i += 2) {
            const float4 q = *(const float4 *)(x + 2 * i);
            const float m0 = p.b * (q.x + q.y), m1 = p.b * (q.z + q.w);
            p.diff[o + i * T] = p.a * (q.y - q.x);
            p.diff[o + (i + 1) * T] = p.a * (q.w - q.z);
            p.avg[o + i * T] = m0;
            p.avg[o + (i + 1) * T] = m1;
            if (cond) { cond[i * T] = m0; cond[(i + 1) * T] = m1; }
        }
        return;
    }
    for (int i = 0; i < p.half; ++i) {
        const float u = x[2 * i * p.s_c], v = x[(2 * i + 1) * p.s_c];
        const float m = p.b * (u + v);
        p.diff[o + i * T] = p.a * (v - u);
        p.avg[o + i * T] = m;
        if (cond) cond[i * T] = m;
    }
}

__global__ __launch_bounds__(256) void haar_merge_kernel(HaarArgs p)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long T = p.T, plane = (long long)p.half * T;
    if (!p.by_column) {
        const long long tq = (T + 3) / 4;
        if (gid >= (long long)p.B * p.half * tq) return;
        const long long t0 = (gid % tq) * 4, i = (gid / tq) % p.half, b = gid / (tq * p.half);
        const long long o = b * plane + i * T + t0;
        const float *m2 = p.avg2 ? p.avg2 + b * p.rows2 * T + i * T + t0 : nullptr;
        float *z0 = p.out + b * p.s_b + 2 * i * p.s_c + t0 * p.s_t, *z1 = z0 + p.s_c;
        if (p.vec) {
            float4 m = *(const float4 *)(p.avg + o);
            const float4 d = *(const float4 *)(p.diff + o);
            if (m2) { const float4 n = *(const float4 *)m2; m.x += n.x; m.y += n.y; m.z += n.z; m.w += n.w; }
            *(float4 *)z0 = make_float4(p.a * m.x - p.b * d.x, p.a * m.y - p.b * d.y, p.a * m.z - p.b * d.z, p.a * m.w - p.b * d.w);
            *(float4 *)z1 = make_float4(p.a * m.x + p.b * d.x, p.a * m.y + p.b * d.y, p.a * m.z + p.b * d.z, p.a * m.w + p.b * d.w);
            return;
        }
        for (int k = 0; k < 4 && t0 + k < T; ++k) {
            float m = p.avg[o + k];
            const float d = p.diff[o + k];
            if (m2) m += m2[k];
            z0[k * p.s_t] = p.a * m - p.b * d;
            z1[k * p.s_t] = p.a * m + p.b * d;
        }
        return;
    }
    if (gid >= (long long)p.B * T) return;
    const long long t = gid % T, b = gid / T;
    const long long o = b * plane + t;
    const float *m2 = p.avg2 ? p.avg2 + b * p.rows2 * T + t : nullptr;
    float *z = p.out + b * p.s_b + t * p.s_t;
    if (p.vec) {                                        // s_c == 1, half even: two pairs per float4
        for (int i = 0; i < p.half; i += 2) {
            float m0 = p.avg[o + i * T], m1 = p.avg[o + (i + 1) * T];
            const float d0 = p.diff[o + i * T], d1 = p.diff[o + (i + 1) * T];
            if (m2) { m0 += m2[i * T]; m1 += m2[(i + 1) * T]; }
            *(float4 *)(z + 2 * i) = make_float4(p.a * m0 - p.b * d0, p.a * m0 + p.b * d0, p.a * m1 - p.b * d1, p.a * m1 + p.b * d1);
        }
        return;
    }
    for (int i = 0; i < p.half; ++i) {
        float m = p.avg[o + i * T];
        const float d = p.diff[o + i * T];
        if (m2) m += m2[i * T];
        z[2 * i * p.s_c] = p.a * m - p.b * d;
        z[(2 * i + 1) * p.s_c] = p.a * m + p.b * d;
    }
}

// how the two Haar kernels walk a strided tensor, and whether 16-byte accesses are safe on every operand
inline void haar_plan(HaarArgs &p, const void *strided, const void *extra)
{
    p.by_column = p.s_c == 1 && p.s_t != 1;
    const bool planes = aligned16(p.diff) && aligned16(p.avg) && p.T % 4 == 0;
    if (p.by_column)
        p.vec = p.half % 2 == 0 && aligned16(strided) && p.s_t % 4 == 0 && p.s_b % 4 == 0;
    else
        p.vec = planes && p.s_t == 1 && aligned16(strided) && p.s_c % 4 == 0 && p.s_b % 4 == 0 && (!extra || aligned16(extra));
}

struct UpArgs {
    const float *h;          // [B, n_mels, F]
    const float *head;       // [B, r0, T] copied to rows [0, r0) (nullable)
    float *out;              // [B, rows, T]; backward: the gradient of that buffer
    float *dh;               // backward: [B, n_mels, F]
    int B, n_mels, F, s, T, rows, r0;
    int vec;
};

// column t reads frames (i0, i1) with weights (w0, w1); i1 == i0 (before the first centre, past the last one, F = 1) means weight 1
__device__ inline void up_source(int t, int s, int F, int &i0, int &i1, float &w0, float &w1)
{
    const int p = 2 * t + 1 - s;
    if (p < 0) { i0 = i1 = 0; w0 = 1.f; w1 = 0.f; return; }
    i0 = p / (2 * s);
    const int r = p - i0 * 2 * s;
    i1 = min(i0 + 1, F - 1);
    w0 = (float)(2 * s - r) / (float)(2 * s);
    w1 = (float)r / (float)(2 * s);
}

__device__ inline float up_value(const float *hrow, int t, int s, int F)
{
    int i0, i1;
    float w0, w1;
    up_source(t, s, F, i0, i1, w0, w1);
    return i1 == i0 ? hrow[i0] : fmaf(hrow[i1], w1, hrow[i0] * w0);
}

// one thread per (item, row of the filled part, 4 columns)
__global__ __launch_bounds__(256) void upsample_kernel(UpArgs p)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long T = p.T, tq = (T + 3) / 4;
    const int first = p.head ? 0 : p.r0, nrows = p.r0 + p.n_mels - first;
    if (gid >= (long long)p.B * nrows * tq) return;
    const int t0 = (int)(gid % tq) * 4, row = first + (int)((gid / tq) % nrows);
    const long long b = gid / (tq * nrows);
    float *out = p.out + (b * p.rows + row) * T + t0;
    if (row < p.r0) {
        const float *src = p.head + (b * p.r0 + row) * T + t0;
        if (p.vec) { *(float4 *)out = *(const float4 *)src; return; }
        for (int k = 0; k < 4 && t0 + k < T; ++k) out[k] = src[k];
        return;
    }
    const float *hrow = p.h + (b * p.n_mels + (row - p.r0)) * p.F;
    if (p.vec) {
        *(float4 *)out = make_float4(up_value(hrow, t0, p.s, p.F), up_value(hrow, t0 + 1, p.s, p.F), up_value(hrow, t0 + 2, p.s, p.F),
                                     up_value(hrow, t0 + 3, p.s, p.F));
        return;
    }
    for (int k = 0; k < 4 && t0 + k < T; ++k) out[k] = up_value(hrow, t0 + k, p.s, p.F);
}

// one thread per (item, mel row, frame): the columns whose (i0, i1) name the frame lie in [s (f - 1), s (f + 2)]
__global__ __launch_bounds__(256) void upsample_bwd_kernel(UpArgs p)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)p.B * p.n_mels * p.F) return;
    const int f = (int)(gid % p.F), m = (int)((gid / p.F) % p.n_mels);
    const long long b = gid / ((long long)p.F * p.n_mels);
    const float *dy = p.out + (b * p.rows + p.r0 + m) * (long long)p.T;
    const long long lo = (long long)p.s * (f - 1), hi = (long long)p.s * (f + 2);
    const int t_lo = (int)(lo < 0 ? 0 : lo), t_hi = (int)(hi > p.T - 1 ? p.T - 1 : hi);
    float acc = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
        int i0, i1;
        float w0, w1;
        up_source(t, p.s, p.F, i0, i1, w0, w1);
        if (i0 == i1) { if (i0 == f) acc += dy[t]; }
        else if (i0 == f) acc = fmaf(w0, dy[t], acc);
        else if (i1 == f) acc = fmaf(w1, dy[t], acc);
    }
    p.dh[gid] = acc;
}

struct PackArgs {
    const float *src;
    float *dst;
    int B, c, T, n_group, off;
    int vec;
};

// one thread per (item, column): the c channels are contiguous in the latent.  unpack = the same walk with the roles swapped
template <bool UNPACK>
__device__ inline void pack_walk(const PackArgs &p)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long T = p.T;
    if (gid >= (long long)p.B * T) return;
    const long long t = gid % T, b = gid / T;
    const long long planar = b * p.c * T + t, latent = (b * T + t) * p.n_group + p.off;
    if (p.vec) {
        for (int ch = 0; ch < p.c; ch += 4) {
            if (UNPACK) {
                const float4 q = *(const float4 *)(p.src + latent + ch);
                p.dst[planar + ch * T] = q.x; p.dst[planar + (ch + 1) * T] = q.y; p.dst[planar + (ch + 2) * T] = q.z; p.dst[planar + (ch + 3) * T] = q.w;
            } else {
                *(float4 *)(p.dst + latent + ch) = make_float4(p.src[planar + ch * T], p.src[planar + (ch + 1) * T], p.src[planar + (ch + 2) * T],
                                                               p.src[planar + (ch + 3) * T]);
            }
        }
        return;
    }
    for (int ch = 0; ch < p.c; ++ch) {
        if (UNPACK) p.dst[planar + ch * T] = p.src[latent + ch];
        else p.dst[latent + ch] = p.src[planar + ch * T];
    }
}

__global__ __launch_bounds__(256) void pack_kernel(PackArgs p) { pack_walk<false>(p); }
__global__ __launch_bounds__(256) void unpack_kernel(PackArgs p) { pack_walk<true>(p); }

inline int pack_check(const float *src, const float *dst, int B, int c, int T, int n_group, int off)
{
    if (!src || !dst || B < 1 || c < 1 || T < 1 || n_group < 1 || off < 0 || off + (long long)c > n_group) return WG_EINVAL;
    return blocks_for((long long)B * T) ? WG_OK : WG_EUNSUPPORTED;
}

// split: diff = a (x1 - x0), avg = b (x0 + x1).  merge: z = a avg -+ b diff.  mode 0 is the model's own map (1, 1/2), mode 1 the other
// kernel's backward (1/2, 1).
inline int haar_coeffs(int mode, float &a, float &b)
{
    if (mode != 0 && mode != 1) return WG_EINVAL;
    a = mode ? 0.5f : 1.f;
    b = mode ? 1.f : 0.5f;
    return WG_OK;
}

}  // namespace mr

extern "C" {

int wg_mr_haar_split(const float *x, int64_t s_b, int64_t s_c, int64_t s_t, int B, int c, int T, int mode, float *diff, float *avg,
                     float *cond, int cond_rows, void *stream)
{
    mr::HaarArgs p = {};
    if (!x || !diff || !avg || B < 1 || c < 2 || (c & 1) || T < 1 || s_b < 0 || s_c < 0 || s_t < 0) return WG_EINVAL;
    if (mr::haar_coeffs(mode, p.a, p.b)) return WG_EINVAL;
    if (cond && cond_rows < c / 2) return WG_EINVAL;
    p.x = x; p.diff = diff; p.avg = avg; p.cond = cond; p.rows2 = cond_rows;
    p.s_b = s_b; p.s_c = s_c; p.s_t = s_t; p.B = B; p.half = c / 2; p.T = T;
    mr::haar_plan(p, x, cond);
    const unsigned nb = mr::blocks_for(p.by_column ? (long long)B * T : (long long)B * p.half * ((T + 3) / 4));
    if (!nb) return WG_EUNSUPPORTED;
    hipLaunchKernelGGL(mr::haar_split_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, p);
    return mr::launched();
}

int wg_mr_haar_merge(const float *avg, const float *avg2, int avg2_rows, const float *diff, int B, int c, int T, int mode, float *out,
                     int64_t o_b, int64_t o_c, int64_t o_t, void *stream)
{
    mr::HaarArgs p = {};
    if (!avg || !diff || !out || B < 1 || c < 2 || (c & 1) || T < 1 || o_b < 0 || o_c < 1 || o_t < 1) return WG_EINVAL;   // (an output: no two elements at one address)
    if (mr::haar_coeffs(mode, p.a, p.b)) return WG_EINVAL;
    if (avg2 && avg2_rows < c / 2) return WG_EINVAL;
    p.avg = (float *)avg; p.diff = (float *)diff; p.avg2 = avg2; p.rows2 = avg2_rows; p.out = out;
    p.s_b = o_b; p.s_c = o_c; p.s_t = o_t; p.B = B; p.half = c / 2; p.T = T;
    mr::haar_plan(p, out, avg2);
    const unsigned nb = mr::blocks_for(p.by_column ? (long long)B * T : (long long)B * p.half * ((T + 3) / 4));
    if (!nb) return WG_EUNSUPPORTED;
    hipLaunchKernelGGL(mr::haar_merge_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, p);
    return mr::launched();
}

static int mr_up_check(const void *h, const void *buf, int B, int n_mels, int F, int s, int T, int rows, int r0)
{
    if (!h || !buf || B < 1 || n_mels < 1 || F < 1 || s < 1 || T < 1 || r0 < 0 || rows < 1 || (long long)r0 + n_mels > rows) return WG_EINVAL;
    if ((long long)F * s > 0x3fffffffLL) return WG_EUNSUPPORTED;                  // 2t + 1 - s and s (f + 2) stay ints
    if (T > (long long)F * s) return WG_ESHAPE;                                   // assert x.size(2) <= y.size(2)
    return WG_OK;
}

int wg_mr_upsample(const float *h, const float *head, int B, int n_mels, int F, int s, int T, float *out, int rows, int r0, void *stream)
{
    const int rc = mr_up_check(h, out, B, n_mels, F, s, T, rows, r0);
    if (rc) return rc;
    if (head && r0 < 1) return WG_EINVAL;
    mr::UpArgs p = {};
    p.h = h; p.head = head; p.out = out; p.B = B; p.n_mels = n_mels; p.F = F; p.s = s; p.T = T; p.rows = rows; p.r0 = r0;
    p.vec = T % 4 == 0 && mr::aligned16(out) && (!head || mr::aligned16(head));
    const unsigned nb = mr::blocks_for((long long)B * (n_mels + (head ? r0 : 0)) * ((T + 3) / 4));
    if (!nb) return WG_EUNSUPPORTED;
    hipLaunchKernelGGL(mr::upsample_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, p);
    return mr::launched();
}

int wg_mr_upsample_backward(const float *dout, int rows, int r0, int B, int n_mels, int F, int s, int T, float *dh, void *stream)
{
    const int rc = mr_up_check(dh, dout, B, n_mels, F, s, T, rows, r0);
    if (rc) return rc;
    mr::UpArgs p = {};
    p.out = (float *)dout; p.dh = dh; p.B = B; p.n_mels = n_mels; p.F = F; p.s = s; p.T = T; p.rows = rows; p.r0 = r0;
    const unsigned nb = mr::blocks_for((long long)B * n_mels * F);
    if (!nb) return WG_EUNSUPPORTED;
    hipLaunchKernelGGL(mr::upsample_bwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, p);
    return mr::launched();
}

int wg_mr_pack(const float *src, int B, int c, int T, int n_group, int off, float *dst, void *stream)
{
    const int rc = mr::pack_check(src, dst, B, c, T, n_group, off);
    if (rc) return rc;
    mr::PackArgs p = {src, dst, B, c, T, n_group, off, 0};
    p.vec = c % 4 == 0 && off % 4 == 0 && n_group % 4 == 0 && mr::aligned16(dst);
    hipLaunchKernelGGL(mr::pack_kernel, dim3(mr::blocks_for((long long)B * T)), dim3(256), 0, (hipStream_t)stream, p);
    return mr::launched();
}

int wg_mr_unpack(const float *src, int B, int c, int T, int n_group, int off, float *dst, void *stream)
{
    const int rc = mr::pack_check(src, dst, B, c, T, n_group, off);
    if (rc) return rc;
    mr::PackArgs p = {src, dst, B, c, T, n_group, off, 0};
    p.vec = c % 4 == 0 && off % 4 == 0 && n_group % 4 == 0 && mr::aligned16(src);
    hipLaunchKernelGGL(mr::unpack_kernel, dim3(mr::blocks_for((long long)B * T)), dim3(256), 0, (hipStream_t)stream, p);
    return mr::launched();
}

}  // extern "C"
