// MelGlow's eval-mode passes as one call each (wg_mg_forward / wg_mg_inverse): MelGlow.forward_computation / reverse_computation
// (model/melglow.py:196-258 upstream) with every module in eval(), from packed weights and one workspace, on one stream in one linear
// chain of launches -- no allocation, no synchronisation, no read-back, no atomics, so the call can be captured and two runs give the
// same bits.  Exact fp32 on the vector ALUs like everything in wg_lvc.h: the result does not depend on WG_PREC_*.
//
// Included at the end of wgflow.hip: it uses the invertible 1x1's device code as it is (lu_kernel at pack time; mix_kernel, squeeze_kernel
// and unsqueeze_kernel on an unpadded plane: a Geo with no halo) and the kernels of wg_lvc.h.
//
// Per flow, in the direction of the pass:
//   run_mix                  x = W x (or W^-1 x) on the flow's channels of the state plane, in place
//   gemm_kernel<false>       h_0 = start . x_a                                                       [B][R][T]
//   gemm_kernel<false>       the predictor's end product straight into the LVC layout                 [depth][B F][2D R radix]
//   lvc_layer_kernel x depth h ping-pong between two planes, skip accumulated in place
//   mg_end_affine_kernel     (log_s, t) = end . skip per element of x_b, the affine map in place, log_s summed per 256 elements
// and once per call: the predictors of ALL flows up to their end products (they read the conditioning alone): the start product and
// 2 * pred_layers grouped products through gemm_kernel<true>, BatchNorm + tanh (+ residual) in the epilogue, batched over the flows
// (1 + 2 pred_layers launches of flows x depth groups instead of that many per flow); squeeze_kernel, mg_logdet_kernel (the partial sums in a fixed order + T log|det W| per flow), unsqueeze_kernel.
#pragma once

namespace {

#define MGF_LU_STRIDE (3 * WG_MAXC * WG_MAXC + 64)      // lu_kernel's slot per matrix: W | W^-1 | log|det W| | its scratch copy

std::atomic<long long> g_mg_pass_calls{0};              // wg_stat_mg_pass_calls
std::atomic<long long> g_mg_layer_launches{0};          // wg_stat_mg_layer_launches

struct MgAffArgs {
    const float *wend;      // [2 ic][S]: rows [0, ic) give log_s, rows [ic, 2 ic) give t
    const float *skip;      // [B][S][T]
    float *X;               // state plane [B][G][T]; x_b = channels [off + ic, off + 2 ic)
    double *part;           // [B][gridDim.x]: this flow's signed sum of log_s over the block's 256 elements
    int S, ic, G, off, T, reverse;
};

// one thread per (channel j of x_b, column t), e = j T + t; blocks past the flow's ic T elements only write their zero partial sum
__global__ __launch_bounds__(256) void mg_end_affine_kernel(MgAffArgs a)
{
    __shared__ double red[256];
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    double sum = 0.0;
    if (e < (long long)a.ic * a.T) {
        const int j = (int)(e / a.T), t = (int)(e % a.T);
        const float *sk = a.skip + (long long)b * a.S * a.T + t;
        float *xb = a.X + ((long long)b * a.G + a.off + a.ic + j) * a.T + t;
        const float *wl = a.wend + (long long)j * a.S, *wt = a.wend + (long long)(a.ic + j) * a.S;
        float ls = 0.f, tt = 0.f;
        for (int s = 0; s < a.S; ++s) {
            const float v = sk[(long long)s * a.T];
            ls = fmaf(wl[s], v, ls);
            tt = fmaf(wt[s], v, tt);
        }
        const float sc = expf(ls), x = xb[0];
        xb[0] = a.reverse ? (x - tt) / sc : x * sc + tt;                             // as affine_plain_kernel
        sum = ls;
    }
    const double tot = mg::block_sum(sum, red);
    if (threadIdx.x == 0) a.part[(long long)b * gridDim.x + blockIdx.x] = a.reverse ? -tot : tot;
}

// logdet[b] = sum over flows and column blocks of the partial sums (thread-strided, then the LDS tree: a fixed order) + coef_T sum_k log|det W_k|
__global__ __launch_bounds__(256) void mg_logdet_kernel(const float *lu, int flows, float coef_T, const double *part, int B, int nblk, float *logdet)
{
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < flows * nblk; i += 256) s += part[((long long)(i / nblk) * B + b) * nblk + i % nblk];
    const double tot = mg::block_sum(s, red);
    if (tid == 0) {
        double w = 0.0;
        for (int k = 0; k < flows; ++k) w += (double)coef_T * lu[(size_t)k * MGF_LU_STRIDE + 2 * WG_MAXC * WG_MAXC];
        logdet[b] = (float)(tot + w);
    }
}

// ---- dimensions, table, packed weights, workspace ----------------------------------------------------------------------------------
struct MgDims {
    int flows, G, every, early, hop, mels, depth, R, D, S, K, H, P, rm;
    int L, HG, Mk, nbn, per_flow;
};
MgDims mg_dims(const wg_mg_config *c)
{
    MgDims d;
    d.flows = c->flows; d.G = c->n_group; d.every = c->n_early_every; d.early = c->n_early_size; d.hop = c->hop; d.mels = c->n_mels;
    d.depth = c->depth; d.R = c->res_ch; d.D = c->dil_ch; d.S = c->skip_ch; d.K = c->radix; d.H = c->pred_ch; d.P = c->pred_layers;
    d.rm = c->reverse_mode != 0;
    d.L = d.hop / d.G;
    d.HG = d.H * d.depth;
    d.Mk = 2 * d.D * d.R * d.K;
    d.nbn = 1 + 2 * d.P;
    d.per_flow = 2 + 2 * d.depth + 1 + 5 + 1 + 10 * d.P;
    return d;
}
inline int mg_flow_off(const MgDims &d, int k) { return d.early * (k / d.every); }       // channels that left before flow k

// configuration alone (no shape): what the packed layout and the table need
int mg_cfg_check(const wg_mg_config *c)
{
    if (!c) return WG_EINVAL;
    if (c->flows < 1 || c->n_group < 2 || c->n_early_every < 1 || c->n_early_size < 0 || c->hop < 1 || c->n_mels < 1 || c->depth < 1 ||
        c->res_ch < 1 || c->dil_ch < 1 || c->skip_ch < 1 || c->radix < 1 || c->pred_ch < 1 || c->pred_layers < 0)
        return WG_EINVAL;
    if (c->flows > WG_MAX_FLOWS || c->n_group > WG_MAXC || c->depth > 16) return WG_EUNSUPPORTED;
    if (c->hop % c->n_group) return WG_EUNSUPPORTED;                   // a frame owns hop / n_group whole columns
    if (!(c->radix & 1)) return WG_EUNSUPPORTED;
    if (c->dil_ch > LVC_MAXD || c->res_ch > LVC_MAXR || c->res_ch * c->radix > LVC_MAXRK) return WG_EUNSUPPORTED;
    if (c->skip_ch > 4096 || c->pred_ch > 4096 || c->n_mels > 65536 || c->pred_layers > 64) return WG_EUNSUPPORTED;
    const MgDims d = mg_dims(c);
    for (int k = 0; k < d.flows; ++k) {
        const int ch = d.G - mg_flow_off(d, k);
        if (ch < 2 || (ch & 1)) return WG_EUNSUPPORTED;                // the coupling halves the flow's channels; the 1x1 mixes 2 .. 32 even
    }
    return WG_OK;
}

struct MgPackFlow {
    size_t start, wo[16], end, pend;                                  // float offsets
};
// The predictors depend on the conditioning alone, so every stage but the last runs for ALL flows in one launch (batch = flows, or
// flows x depth groups): their weights and BatchNorm blocks are laid out stage by stage with the flows contiguous.
//   pstart [flows][H G][mels]; blk[j] [flows][H G][H]; bn[j]: mean double[flows H G] | invstd double[flows H G] | gamma | beta
struct MgPack {
    size_t lu, scratch, pstart, bn[1 + 2 * 64], blk[2 * 64], total;
    std::vector<MgPackFlow> f;
};
MgPack mg_pack_layout(const MgDims &d)
{
    MgPack L;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += (n + 3) / 4 * 4; return o; };       // 16-byte granules (the doubles)
    L.lu = take((size_t)d.flows * MGF_LU_STRIDE);
    L.scratch = take(d.HG);                                                                     // bn_stats_kernel's third output
    L.pstart = take((size_t)d.flows * d.HG * d.mels);
    for (int j = 0; j < d.nbn; ++j) L.bn[j] = take((size_t)6 * d.flows * d.HG);
    for (int j = 0; j < 2 * d.P; ++j) L.blk[j] = take((size_t)d.flows * d.HG * d.H);
    L.f.resize(d.flows);
    for (int k = 0; k < d.flows; ++k) {
        MgPackFlow &f = L.f[k];
        const int ic = (d.G - mg_flow_off(d, k)) / 2;
        f.start = take((size_t)d.R * ic);
        for (int l = 0; l < d.depth; ++l) f.wo[l] = take((size_t)(l == d.depth - 1 ? d.S : d.R + d.S) * d.D);
        f.end = take((size_t)2 * ic * d.S);
        f.pend = take((size_t)d.depth * d.Mk * d.H);
    }
    L.total = off;
    return L;
}

struct MgWs {
    size_t X, h0, h1, skip, pa, pb, pc, wp, part, total;       // float offsets
    int T, Fr, nblk;
};
MgWs mg_ws_layout(const MgDims &d, int B, int N)
{
    MgWs W;
    W.T = N / d.G; W.Fr = N / d.hop; W.nblk = (int)(((long long)W.T * (d.G / 2) + 255) / 256);       // the widest flow's x_b
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += (n + 3) / 4 * 4; return o; };
    const size_t ncol = (size_t)B * W.Fr;
    W.part = take((size_t)2 * d.flows * B * W.nblk);           // doubles
    W.X = take((size_t)B * d.G * W.T);
    W.h0 = take((size_t)B * d.R * W.T);
    W.h1 = take((size_t)B * d.R * W.T);
    W.skip = take((size_t)B * d.S * W.T);
    W.pa = take((size_t)d.flows * d.HG * ncol);                  // the predictors' activations, every flow's: [flows][H G][B Fr]
    W.pb = take((size_t)d.flows * d.HG * ncol);
    W.pc = take((size_t)d.flows * d.HG * ncol);
    W.wp = take((size_t)d.depth * ncol * d.Mk);
    W.total = off;
    return W;
}

// a BatchNorm block of the packed buffer, from channel `first` on (`total` channels in the block)
struct MgBn {
    const double *mean, *invstd;
    const float *gamma, *beta;
};
MgBn mg_bn(const float *block, size_t total, size_t first)
{
    MgBn b;
    b.mean = (const double *)block + first; b.invstd = (const double *)block + total + first;
    b.gamma = block + 4 * total + first; b.beta = block + 5 * total + first;
    return b;
}

// one product through gemm_kernel, never cut along K (the epilogue form has no second launch)
void mg_gemm(Ctx &cx, const wg_mg_gemm_desc &d, const float *A, const float *Bm, float *C, const MgBn *bn = nullptr, const float *res = nullptr)
{
    mg::GemmArgs p;
    p.d = d; p.A = A; p.B = Bm; p.D = nullptr; p.C = C;
    p.splits = 1; p.kc = (d.K + MG_BK - 1) / MG_BK * MG_BK; p.ws = nullptr;
    p.bn_mean = p.bn_invstd = nullptr; p.bn_gamma = p.bn_beta = p.bn_res = nullptr;
    const dim3 grid((unsigned)((d.N + MG_BN - 1) / MG_BN), (unsigned)((d.M + MG_BM - 1) / MG_BM), (unsigned)d.batch);
    if (bn) {
        p.bn_mean = bn->mean; p.bn_invstd = bn->invstd; p.bn_gamma = bn->gamma; p.bn_beta = bn->beta; p.bn_res = res;
        WG_LAUNCH(cx, mg::gemm_kernel<true>, grid, dim3(256), 0, p);
    } else {
        WG_LAUNCH(cx, mg::gemm_kernel<false>, grid, dim3(256), 0, p);
    }
}
wg_mg_gemm_desc mg_desc(int M, int N, int K, int batch, int N1)
{
    wg_mg_gemm_desc g;
    memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.K = K; g.batch = batch; g.N1 = N1; g.K1 = K; g.alpha = 1.f; g.beta = 1.f;
    return g;
}

// Predictor.forward in eval() up to its end product, for the nf flows from flow0 on in 1 + 2 P launches: h [B][mels][F] (its first Fr
// frames) -> the returned plane (one of pa / pb / pc) [nf][H G][B Fr].  The epilogue's channel is batch * M + m = (flow, group, row).
float *mg_predictor(Ctx &cx, const MgDims &d, const float *pk, const MgPack &L, int flow0, int nf, const float *h, int B, int Fr, int F,
                    float *pa, float *pb, float *pc)
{
    const int ncol = B * Fr;
    const size_t total = (size_t)d.flows * d.HG, first = (size_t)flow0 * d.HG;
    wg_mg_gemm_desc g = mg_desc(d.HG, ncol, d.mels, nf, Fr);                 // start: columns n = b Fr + f read through h's strides
    g.a_m = d.mels; g.a_k = 1; g.a_b = (int64_t)d.HG * d.mels;
    g.b_k = F; g.b_n = 1; g.b_n2 = (int64_t)d.mels * F;                      // (b_b = 0: every flow reads the same conditioning)
    g.c_m = ncol; g.c_n = 1; g.c_n2 = Fr; g.c_b = (int64_t)d.HG * ncol;
    MgBn bn = mg_bn(pk + L.bn[0], total, first);
    mg_gemm(cx, g, pk + L.pstart + first * d.mels, h, pa, &bn);
    float *P = pa, *s1 = pb, *Pn = pc;
    for (int r = 0; r < d.P; ++r) {
        wg_mg_gemm_desc q = mg_desc(d.H, ncol, d.H, nf * d.depth, ncol);     // grouped 1x1: one group per (flow, layer of the WN)
        q.a_m = d.H; q.a_k = 1; q.a_b = (int64_t)d.H * d.H;
        q.b_k = ncol; q.b_n = 1; q.b_b = (int64_t)d.H * ncol;
        q.c_m = ncol; q.c_n = 1; q.c_b = (int64_t)d.H * ncol;
        MgBn b1 = mg_bn(pk + L.bn[1 + 2 * r], total, first), b2 = mg_bn(pk + L.bn[2 + 2 * r], total, first);
        mg_gemm(cx, q, pk + L.blk[2 * r] + first * d.H, P, s1, &b1);
        mg_gemm(cx, q, pk + L.blk[2 * r + 1] + first * d.H, s1, Pn, &b2, P);
        std::swap(P, Pn);
    }
    return P;
}

// the predictor's end product of one flow: wp[g][n][m] = sum_k E[g Mk + m][k] P[g H + k][n], launched transposed (rows = columns n,
// columns = kernel elements m) so that neighbouring lanes write neighbouring kernel elements; the fma chain over k is the same
void mg_pred_end(Ctx &cx, const MgDims &d, const float *E, const float *P, int ncol, float *wp)
{
    wg_mg_gemm_desc e = mg_desc(ncol, d.Mk, d.H, d.depth, d.Mk);
    e.a_m = 1; e.a_k = ncol; e.a_b = (int64_t)d.H * ncol;
    e.b_k = 1; e.b_n = d.H; e.b_b = (int64_t)d.Mk * d.H;
    e.c_m = d.Mk; e.c_n = 1; e.c_b = (int64_t)ncol * d.Mk;
    mg_gemm(cx, e, P, E, wp);
}

void mg_layer(Ctx &cx, const MgDims &d, int dilation, int first, int last, const float *h, const float *w, const float *wo, int B, int T, int Fr,
              float *hn, float *skip)
{
    mg::LvcLayerArgs p;
    p.a.R = d.R; p.a.D = d.D; p.a.K = d.K; p.a.dil = dilation; p.a.L = T / Fr; p.a.T = T; p.a.F = Fr;
    p.S = d.S; p.first = first; p.last = last; p.h = h; p.W = w; p.wo = wo; p.hn = hn; p.skip = skip;
    WG_LAUNCH(cx, mg::lvc_layer_kernel, dim3(Fr, B), dim3(256), 0, p);
    if (!cx.err) g_mg_layer_launches.fetch_add(1, std::memory_order_relaxed);
}

Geo mg_plain_geo(int B, int T)
{
    Geo g;
    g.B = B; g.T = T; g.Tt = T; g.H = 0; g.P = T; g.rows = 0;               // no halo: paddr is [B][channels][T]
    return g;
}

// order: flows ascending (forward_computation) or descending (reverse_computation); the arithmetic of every block is its
// forward_computation unless reverse_mode swaps it (base.py Reversible: a reverse_mode model's blocks are built with reverse_mode too)
int mg_pass(const wg_mg_config *cf, const void *packed, const float *in, const float *h, int B, int N, int F, float *out, float *logdet,
            void *wsv, size_t ws_bytes, void *stream, int descending)
{
    if (!cf || !packed || !in || !h || !out || !logdet || !wsv) return WG_EINVAL;
    const int rc = wg_mg_check(cf, B, N, F);
    if (rc) return rc;
    const MgDims d = mg_dims(cf);
    const MgWs W = mg_ws_layout(d, B, N);
    if (W.total * sizeof(float) > ws_bytes) return WG_EWORKSPACE;
    const MgPack L = mg_pack_layout(d);
    const float *pk = (const float *)packed;
    float *ws = (float *)wsv;
    const int T = W.T, Fr = W.Fr;
    const int reverse = (descending != 0) != (d.rm != 0);                      // the blocks' arithmetic: x -> z (0) or z -> x (1)
    Ctx cx = {(hipStream_t)stream, 0, 0};
    const Geo g = mg_plain_geo(B, T);
    const dim3 cgrid((T + 255) / 256, B);
    double *part = (double *)(ws + W.part);
    WG_LAUNCH(cx, squeeze_kernel, cgrid, dim3(256), 0, in, pref(ws + W.X, d.G), g, d.G, N);
    const float *P = mg_predictor(cx, d, pk, L, 0, d.flows, h, B, Fr, F, ws + W.pa, ws + W.pb, ws + W.pc);
    for (int q = 0; q < d.flows; ++q) {
        const int k = descending ? d.flows - 1 - q : q;
        const MgPackFlow &f = L.f[k];
        const int off = mg_flow_off(d, k), c = d.G - off, ic = c / 2;
        const float *lu = pk + L.lu + (size_t)k * MGF_LU_STRIDE;
        if (!descending) run_mix(cx, g, pref(ws + W.X, d.G, off), c, lu + (reverse ? WG_MAXC * WG_MAXC : 0), 0);
        wg_mg_gemm_desc s = mg_desc(d.R, T, ic, B, T);                          // h_0 = start . x_a, batched over items
        s.a_m = ic; s.a_k = 1;
        s.b_k = T; s.b_n = 1; s.b_b = (int64_t)d.G * T;
        s.c_m = T; s.c_n = 1; s.c_b = (int64_t)d.R * T;
        mg_gemm(cx, s, pk + f.start, ws + W.X + (size_t)off * T, ws + W.h0);
        mg_pred_end(cx, d, pk + f.pend, P + (size_t)k * d.HG * B * Fr, B * Fr, ws + W.wp);
        float *hc = ws + W.h0, *hn = ws + W.h1;
        for (int l = 0; l < d.depth; ++l) {
            mg_layer(cx, d, 1 << l, l == 0, l == d.depth - 1, hc, ws + W.wp + (size_t)l * B * Fr * d.Mk, pk + f.wo[l], B, T, Fr, hn, ws + W.skip);
            std::swap(hc, hn);
        }
        MgAffArgs a;
        a.wend = pk + f.end; a.skip = ws + W.skip; a.X = ws + W.X; a.part = part + (size_t)k * B * W.nblk;
        a.S = d.S; a.ic = ic; a.G = d.G; a.off = off; a.T = T; a.reverse = reverse;
        WG_LAUNCH(cx, mg_end_affine_kernel, dim3(W.nblk, B), dim3(256), 0, a);
        if (descending) run_mix(cx, g, pref(ws + W.X, d.G, off), c, lu + (reverse ? WG_MAXC * WG_MAXC : 0), 0);
    }
    WG_LAUNCH(cx, mg_logdet_kernel, dim3(B), dim3(256), 0, pk + L.lu, d.flows, reverse ? -(float)T : (float)T, (const double *)part, B, W.nblk,
              logdet);
    WG_LAUNCH(cx, unsqueeze_kernel, cgrid, dim3(256), 0, pref(ws + W.X, d.G), out, g, d.G, N);
    if (!cx.err) g_mg_pass_calls.fetch_add(1, std::memory_order_relaxed);
    return cx.err;
}

}  // namespace

extern "C" {

long long wg_stat_mg_pass_calls(void) { return g_mg_pass_calls.load(std::memory_order_relaxed); }
long long wg_stat_mg_layer_launches(void) { return g_mg_layer_launches.load(std::memory_order_relaxed); }

int wg_mg_check(const wg_mg_config *cf, int B, int N, int F)
{
    int rc = mg_cfg_check(cf);
    if (rc) return rc;
    if (B < 1 || N < 1 || F < 1) return WG_EINVAL;
    if (N % cf->hop) return WG_ESHAPE;                                  // whole frames only
    const int Fr = N / cf->hop, T = N / cf->n_group;
    if (F < Fr) return WG_ESHAPE;                                       // the conditioning is shorter than the audio
    const MgDims d = mg_dims(cf);
    for (int l = 0; l < d.depth; ++l) {
        const wg_lvc_dims ld = {d.R, d.D, d.K, 1 << l};
        rc = wg_lvc_check(&ld, B, T, Fr);
        if (rc) return rc;
    }
    if ((long long)B * Fr > 65535LL * MG_BM) return WG_EUNSUPPORTED;    // the end product's row tiles are a grid's y axis
    if ((long long)d.mels * F > 0x7fffffffLL || (long long)B * d.G * T > 0x7fffffffLL) return WG_EUNSUPPORTED;
    return WG_OK;
}

int wg_mg_param_count(const wg_mg_config *cf)
{
    if (mg_cfg_check(cf)) return 0;
    const MgDims d = mg_dims(cf);
    return d.flows * (1 + d.per_flow);
}

size_t wg_mg_packed_bytes(const wg_mg_config *cf)
{
    if (mg_cfg_check(cf)) return 0;
    return mg_pack_layout(mg_dims(cf)).total * sizeof(float);
}

size_t wg_mg_workspace_bytes(const wg_mg_config *cf, int B, int N)
{
    if (mg_cfg_check(cf) || B < 1 || N < 1 || N % cf->hop) return 0;
    if (wg_mg_check(cf, B, N, N / cf->hop)) return 0;
    return mg_ws_layout(mg_dims(cf), B, N).total * sizeof(float);
}

int wg_mg_pack_weights(const wg_mg_config *cf, const void *const *table, const float *bn_eps, void *packed, void *stream)
{
    int rc = mg_cfg_check(cf);
    if (rc) return rc;
    if (!table || !packed) return WG_EINVAL;
    const MgDims d = mg_dims(cf);
    const int n = d.flows * (1 + d.per_flow);
    for (int i = 0; i < n; ++i) {                                       // only a weight_g may be absent
        const int j = i < d.flows ? -1 : (i - d.flows) % d.per_flow;
        const bool is_g = j >= 0 && j < 2 + 2 * d.depth && !(j & 1);
        if (!table[i] && !is_g) return WG_EINVAL;
    }
    const MgPack L = mg_pack_layout(d);
    float *pk = (float *)packed;
    Ctx cx = {(hipStream_t)stream, 0, 0};
    auto T = [&](int i) { return (const float *)table[i]; };
    auto copy = [&](size_t dst, const float *src, size_t count) {
        if (!cx.err && hipMemcpyAsync(pk + dst, src, count * sizeof(float), hipMemcpyDeviceToDevice, cx.st) != hipSuccess) cx.err = WG_ELAUNCH;
    };
    auto wnorm = [&](size_t dst, const float *gp, const float *vp, int rows, int cols) {     // w = g v / ||v||, or the plain weight
        if (!gp) copy(dst, vp, (size_t)rows * cols);
        else WG_LAUNCH(cx, mg::wnorm_kernel, dim3(rows), dim3(256), 0, gp, vp, cols, pk + dst);
    };
    LuArgs lu;
    lu.n = d.flows; lu.out = pk + L.lu; lu.ostride = MGF_LU_STRIDE;
    for (int k = 0; k < d.flows; ++k) { lu.job[k].W = T(k); lu.job[k].c = d.G - mg_flow_off(d, k); }
    WG_LAUNCH(cx, lu_kernel, dim3((d.flows + 63) / 64), dim3(64), 0, lu);
    for (int k = 0; k < d.flows; ++k) {
        const MgPackFlow &f = L.f[k];
        const int base = d.flows + k * d.per_flow, ic = (d.G - mg_flow_off(d, k)) / 2;
        wnorm(f.start, T(base), T(base + 1), d.R, ic);
        for (int l = 0; l < d.depth; ++l)
            wnorm(f.wo[l], T(base + 2 + 2 * l), T(base + 3 + 2 * l), l == d.depth - 1 ? d.S : d.R + d.S, d.D);
        const int e = base + 2 + 2 * d.depth;
        copy(f.end, T(e), (size_t)2 * ic * d.S);
        copy(L.pstart + (size_t)k * d.HG * d.mels, T(e + 1), (size_t)d.HG * d.mels);
        copy(f.pend, T(e + 6), (size_t)d.depth * d.Mk * d.H);
        for (int j = 0; j < d.nbn; ++j) {
            // the BatchNorm entries (weight, bias, running_mean, running_var) of norm j: the start's, then two per residual block
            const int bnp = j == 0 ? e + 2 : e + 7 + 10 * ((j - 1) / 2) + ((j - 1) & 1 ? 6 : 1);
            const float eps = bn_eps ? bn_eps[k * d.nbn + j] : 1e-5f;
            const size_t total = (size_t)d.flows * d.HG, first = (size_t)k * d.HG;
            double *mean = (double *)(pk + L.bn[j]) + first;
            WG_LAUNCH(cx, mg::bn_stats_kernel, dim3(d.HG), dim3(256), 0, (const float *)nullptr, 1, eps, 0, T(bnp + 2), T(bnp + 3), mean, mean + total,
                      pk + L.scratch);
            copy(L.bn[j] + 4 * total + first, T(bnp), d.HG);
            copy(L.bn[j] + 5 * total + first, T(bnp + 1), d.HG);
        }
        for (int r = 0; r < d.P; ++r) {
            copy(L.blk[2 * r] + (size_t)k * d.HG * d.H, T(e + 7 + 10 * r), (size_t)d.HG * d.H);
            copy(L.blk[2 * r + 1] + (size_t)k * d.HG * d.H, T(e + 7 + 10 * r + 5), (size_t)d.HG * d.H);
        }
    }
    return cx.err;
}

int wg_mg_forward(const wg_mg_config *cf, const void *packed, const float *audio, const float *h, int B, int N, int F, float *z, float *logdet,
                  void *ws, size_t ws_bytes, void *stream)
{
    return mg_pass(cf, packed, audio, h, B, N, F, z, logdet, ws, ws_bytes, stream, 0);
}

int wg_mg_inverse(const wg_mg_config *cf, const void *packed, const float *z, const float *h, int B, int N, int F, float *x, float *logdet,
                  void *ws, size_t ws_bytes, void *stream)
{
    return mg_pass(cf, packed, z, h, B, N, F, x, logdet, ws, ws_bytes, stream, 1);
}

int wg_mg_layer_apply(const wg_lvc_dims *ld, int skip_ch, int first, int last, const float *h, const float *w, const float *wo, int B, int T, int F,
                      float *h_next, float *skip, void *stream)
{
    const int rc = wg_lvc_check(ld, B, T, F);
    if (rc) return rc;
    if (skip_ch < 1 || !h || !w || !wo || !skip || (!last && !h_next) || h_next == h) return WG_EINVAL;
    MgDims d;
    memset(&d, 0, sizeof(d));
    d.R = ld->res_ch; d.D = ld->dil_ch; d.K = ld->radix; d.S = skip_ch;
    Ctx cx = {(hipStream_t)stream, 0, 0};
    mg_layer(cx, d, ld->dilation, first != 0, last != 0, h, w, wo, B, T, F, h_next, skip);
    return cx.err;
}

int wg_mg_predictor_apply(const wg_mg_config *cf, const void *packed, int flow, const float *h, int B, int Fr, int F, float *kernels, void *wsv,
                          size_t ws_bytes, void *stream)
{
    int rc = mg_cfg_check(cf);
    if (rc) return rc;
    if (!packed || !h || !kernels || !wsv || B < 1 || Fr < 1 || F < Fr || flow < 0 || flow >= cf->flows) return WG_EINVAL;
    if ((long long)B * Fr > 65535LL * MG_BM || (long long)cf->n_mels * F > 0x7fffffffLL) return WG_EUNSUPPORTED;
    const MgDims d = mg_dims(cf);
    const size_t plane = ((size_t)d.HG * B * Fr + 3) / 4 * 4;
    if (3 * plane * sizeof(float) > ws_bytes) return WG_EWORKSPACE;
    const MgPack L = mg_pack_layout(d);
    float *ws = (float *)wsv;
    Ctx cx = {(hipStream_t)stream, 0, 0};
    const float *P = mg_predictor(cx, d, (const float *)packed, L, flow, 1, h, B, Fr, F, ws, ws + plane, ws + 2 * plane);
    mg_pred_end(cx, d, (const float *)packed + L.f[flow].pend, P, B * Fr, kernels);
    return cx.err;
}

}  // extern "C"
