/*
 * wgflow.h -- C ABI of the MI355X-native WaveGlow flow engine (libwgflow.so).
 *
 * This is the drop-in boundary for the hot path of yoyololicon/constant-memory-waveglow:
 * every entry point replaces a specific piece of the reference's Python/ATen path (cited
 * below as path:line under the upstream repo).  Plain C types only: device pointers, sizes,
 * a stream handle.  No allocation, no global state: every call works inside a caller-provided
 * workspace whose size comes from the matching *_bytes() query, is re-entrant per stream, and
 * only ENQUEUES work on `stream` (hipStream_t passed as void*; NULL = the default stream).
 * All tensors are float32, contiguous, device resident unless a parameter says "host".
 *
 * Return value: 0 on success, a negative WG_E* code otherwise (wg_strerror() names it).
 *
 * Parameter table ("params"): an array of device pointers in the order of the reference
 * model's named_parameters():
 *     [0] upsampler.bias [n_mels]   [1] upsampler.weight_g [n_mels,1,1]   [2] upsampler.weight_v [n_mels,1,K]
 *     [3 .. 3+flows)                invconv1x1.{k}.weight [c_k,c_k,1]
 *     then per flow k, 4+4*depth+1 entries:
 *         V.weight_g, V.weight_v, start.weight_g, start.weight_v,
 *         layers.{i}.W.weight_g, .W.weight_v, .W_o.weight_g, .W_o.weight_v   (i = 0..depth-1),
 *         end.weight
 * A NULL weight_g entry means the convolution carries a plain weight in its weight_v slot
 * (what the module looks like after utils.remove_weight_norms, utils.py:9-11).
 * The gradient table ("grads") has the same order and shapes; NULL entries are skipped.
 */
#ifndef WGFLOW_H
#define WGFLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WG_OK 0
#define WG_EINVAL (-1)      /* bad argument / unsupported shape */
#define WG_ESHAPE (-2)      /* audio length not a multiple of n_group, or mel too short (waveglow.py:156 assert) */
#define WG_EUNSUPPORTED (-3)/* valid for the reference but outside this engine's kernels */
#define WG_ELAUNCH (-4)     /* a HIP launch failed */
#define WG_EWORKSPACE (-5)  /* workspace too small */

/* Arithmetic of the matrix contractions; every tensor in memory is fp32 in both modes.
 *   WG_PREC_F32    v_mfma_f32_32x32x2_f32: bit-exact fp32 fma chains.
 *   WG_PREC_BF16X3 each fp32 operand is split into bf16 hi + lo and a*b is evaluated as a_lo*b_hi + a_hi*b_lo + a_hi*b_hi
 *                  on the bf16 matrix pipe with fp32 accumulation (drops a_lo*b_lo, 2^-16 of a product).
 *   WG_PREC_BF16X3_PLANES  same arithmetic; producers additionally keep every MFMA operand tensor pre-split in bf16 hi/lo
 *                  "S-planes" (wg_gemm16s.h), so the contraction kernels do no conversion work. */
#define WG_PREC_F32 0
#define WG_PREC_BF16X3 1
#define WG_PREC_BF16X3_PLANES 2

/* Constructor arguments of model.WaveGlow (model/waveglow.py:109-118) after the arithmetic of
 * :125-129 (upsampler geometry).  WN arguments are the **kwargs forwarded to WN (waveglow.py:50-59). */
typedef struct wg_config {
    int32_t n_flows, n_group, n_early_every, n_early_size, n_mels;
    int32_t up_stride, up_kernel, up_pad;            /* ConvTranspose1d(n_mels,n_mels,K,stride,pad,groups=n_mels) */
    int32_t res_ch, dil_ch, skip_ch, depth, radix;   /* WN: residual/dilation/skip channels, layers, kernel size (odd, <= 9) */
    int32_t precision;                               /* WG_PREC_* : arithmetic of the MFMA contractions (not upstream) */
    int32_t reverse_mode;                            /* WaveGlow(reverse_mode=...) (waveglow.py:116, base.py:20-28): wg_forward is what
                                                        model.forward computes in that architecture, wg_inverse what model.reverse does */
    int32_t keep_activations;                        /* WaveGlow(memory_efficient=False) (waveglow.py:118, efficient_modules.py:33-35,71-75):
                                                        wg_forward / wg_train_step run in the MODE-1 workspace and leave every flow's WN layers
                                                        there; wg_backward with the same workspace reads them instead of recomputing each WN.
                                                        The caller guarantees nothing else used that workspace in between.  0 = the
                                                        constant-memory scheme (only one flow's layers exist at a time). */
    int32_t bias;                                    /* WN(bias=True) (waveglow.py:58): every conv of every WN carries a bias.  The WN's
                                                        part of the parameter table then continues behind `end.weight` with V.bias,
                                                        start.bias, depth x (layers.i.W.bias, layers.i.W_o.bias), end.bias */
} wg_config;

/* Dimensions of one WN as AffineCouplingBlock builds it (efficient_modules.py:58-65, waveglow.py:50-59). */
typedef struct wg_wn_dims {
    int32_t in_ch, aux_ch, res_ch, dil_ch, skip_ch, depth, radix;
    int32_t precision;                               /* WG_PREC_* */
    int32_t bias;                                    /* WN(bias=True): see wg_config.bias (the block-level table grows the same way) */
} wg_wn_dims;

const char *wg_strerror(int code);
/* ABI revision of this header (2: wg_config gained keep_activations; 3: wg_nll_loss / wg_train_step produce the logged
 * training scalars and take their scratch from the caller, wg_melspec returns the power spectrogram on request, wg_wf_config gained
 * use_conv1x1, wg_wf_upsample; 4: wg_timer_create(-1, ..) times every kernel class, wg_timer_read_info, wg_stat_wgrad16t_launches,
 * wg_wf_* accept every WG_PREC_*; 5: wg_config and wg_wn_dims gained bias; 6: wg_stat_layer_launches, the workspaces carry the one-launch
 * layer's hand-off counters, wg_layer_apply / wg_layer_workspace_bytes, wg_wf_wn_apply; 7: wg_wf_config gained bias; 8: wg_timer_read_name,
 * wg_box_probe / wg_box_probe_bytes, wg_stat_layerg_launches, wg_stat_gate_split_launches,
 * wg_wf_wn_backward, wg_layer_backward / wg_layer_backward_workspace_bytes, wg_affine_apply / wg_affine_backward; 9: wg_reload_env,
 * wg_stat_gate_part_launches, wg_wsr_cond_pre; 10: wg_mg_bn_* pass mean and 1 / std as double).  A binding built against another
 * revision must not pass its structs: the Python loader compares this with its own ABI_VERSION and refuses the library otherwise. */
#define WG_ABI_VERSION 10
int wg_abi_version(void);
/* Developer switches (WG_G192, WG_G192_SPLITK, WG_LOWRANK, WG_TW_FROM_GATE, WG_START_FOLD, WG_LAYER_G, WG_LAYER_MIN_CHUNKS, WG_LAYER_FUSION,
 * WG_LAYER_FUSION_BIG, WG_INV_SEAM: A/B switches between
 * kernels that compute the same thing, csrc/wgflow.hip EnvSw) are read from the environment ONCE per process, at the first call that needs
 * one; a caller that changes one afterwards -- a test, an A/B run -- calls this to have them read again.  Not to be called while
 * another thread is inside the library.  No counterpart upstream. */
void wg_reload_env(void);

/* Diagnostics (no counterpart upstream; the reference times with wall-clock time(), inference.py:39-53): while a
 * timer is attached, every launch of ONE kernel class is bracketed with HIP events on its launch stream, so a
 * benchmark can read that kernel's per-launch durations over the very steps it times.  Process-wide: attach from
 * one thread, detach (attach NULL) before destroying. */
#define WG_K_CONV_STORE 0    /* convgemm, plain / accumulate epilogue: start, dgrad (W^T), V^T, W_end^T, W_start^T */
#define WG_K_CONV_GATE 1     /* convgemm, dilated conv + conditioning + tanh*sigmoid gate   (the dominant kernel) */
#define WG_K_CONV_RESSKIP 2  /* convgemm, W_o + residual/skip epilogue */
#define WG_K_CONV_DGATE 3    /* convgemm, W_o^T + gate backward */
#define WG_K_WGRAD 4         /* weight-gradient kernel */
#define WG_K_LAYER 5         /* convlayer16q_kernel: a layer's gate conv + residual product in one persistent launch (reported as M = gate rows,
                              * K = gate K + residual K * residual rows / gate rows, so that 2 M K columns = the launch's FLOPs) */
#define WG_K_THIN 6          /* the byte-bound passes of the rank-2ic skip path: WN's end conv from the gate planes or from the gate convs' partial rows
                              * (M = 2 ic, K = the channels or rows it adds), and P_l = G gate_l^T over the gate planes (M = 2 ic, K = depth x dil_ch) */
void *wg_timer_create(int kernel_id, int capacity);   /* kernel_id < 0: every class above */
void  wg_timer_attach(void *timer);
int   wg_timer_count(void *timer);
int   wg_timer_read(void *timer, float *ms, int n);   /* after a stream sync; returns the number written */
/* five values per recorded launch: class (WG_K_*), M, K, columns of the product (2 M K columns = its algorithmic FLOPs; a paired
 * weight-gradient launch reports M = the summed sizes of its gradients, K = 1), algorithmic HBM bytes (every operand plane once, the
 * weights, the outputs and auxiliary planes of the epilogue); launches that are not conv / weight-gradient products report zeros */
int   wg_timer_read_info(void *timer, long long *info, int n);
/* the kernel expression of recorded launch `index` as written at its launch site in csrc/wgflow.hip, e.g.
 * "(convgemm16q_kernel<EPI_GATE_SO, 2, 2>)" (template arguments by name, defaulted ones absent): which instantiation RAN.  Returns the
 * name's length (it is truncated to n - 1 characters), or a negative error */
int   wg_timer_read_name(void *timer, int index, char *buf, int n);
void  wg_timer_destroy(void *timer);
/* Box calibration (no counterpart upstream): a fixed matrix-pipe + LDS loop without global traffic on random data (csrc/wg_probe.h), run
 * back to back for about `ms` milliseconds on `stream`.  out[0] = issued TFLOP/s, out[1] = the clock held inside the kernel (GHz),
 * out[2] = ms per launch.  The boxes of a pool differ by a few per cent on exactly this loop; a benchmark line that carries these
 * numbers tells a slower box from a slower build.  scratch: wg_box_probe_bytes() bytes of device memory.  Synchronises the stream. */
size_t wg_box_probe_bytes(void);
int    wg_box_probe(void *scratch, int ms, double *out, void *stream);
/* diagnostics: how many times this process has launched wgrad16t_kernel (the one-workgroup-per-CU weight-gradient kernel; shapes
 * without a plan take wgrad16s_pair_kernel) -- lets a test assert which kernel a shape ran on */
long long wg_stat_wgrad16t_launches(void);
/* diagnostics: launches of convlayer16h_kernel (ONE launch per WN layer: gate conv -> gate -> W_o -> residual / skip, wg_layer16h.h; small grids
 * only -- single-utterance synthesis, WaveFlow's row steps); larger shapes take two launches per layer */
long long wg_stat_layer_launches(void);
/* diagnostics: launches of convlayer16g_kernel (csrc/wg_gemm16g.h: a layer's gate conv and residual product in one launch on 256 x 192 tiles of
 * flattened columns, a workgroup owning whole column tiles -- the training shapes; default on, env WG_LAYER_G=0 switches it off) */
long long wg_stat_layerg_launches(void);
/* diagnostics: gate convs that ran cut along K (convgemm16g_kernel<8> writes S partial 256 x 192 tiles per output tile into the workspace,
 * gate_finish16g_kernel sums them in a fixed order and applies the gate): shapes whose column tiles fill a fraction 1/S of the CUs and
 * whose K is long -- WSRGlow's 512 x 4432 gate conv at 12 x 512 columns; env WG_G192_SPLITK=0 switches it off */
long long wg_stat_gate_split_launches(void);
/* diagnostics: gate convs launched with the partial rows of WN's `out` (csrc/wg_gemm16g.h, wgg_gate_nb: the rank-2ic form of the skip
 * path, csrc/wgflow.hip lowrank_on / gate_parts_on; env WG_LOWRANK=0 switches the form off) -- lets a test assert that a shape took it */
long long wg_stat_gate_part_launches(void);

/* ---- sizes -------------------------------------------------------------------------------- */
int    wg_param_count(const wg_config *cfg);                 /* entries of the parameter table */
size_t wg_packed_bytes(const wg_config *cfg);                /* materialised-weight buffer of the model */
/* mode 0: forward / inverse (2 activation planes per WN);  mode 1: backward (all layers kept for ONE flow) */
size_t wg_workspace_bytes(const wg_config *cfg, int B, int N, int mode);
int    wg_wn_param_count(const wg_wn_dims *d);
size_t wg_wn_packed_bytes(const wg_wn_dims *d);
size_t wg_coupling_workspace_bytes(const wg_wn_dims *d, int B, int T, int mode);
size_t wg_invconv_workspace_bytes(int c, int B, int T);

/* Workspaces keep zero halos between calls; zero a freshly allocated one ONCE with this. */
int wg_workspace_init(void *ws, size_t bytes, void *stream);

/* ---- weights ------------------------------------------------------------------------------ */
/* Replaces the weight_norm forward pre-hooks (utils.py:14-16; w = g*v/||v||, recomputed on every module
 * call upstream) and the per-call logdet/inverse of the 1x1 weights (efficient_modules.py:221,235):
 * materialises every effective weight ONCE per step in the layouts the kernels read. */
int wg_pack_weights(const wg_config *cfg, const void *const *params, void *packed, void *stream);
int wg_wn_pack_weights(const wg_wn_dims *d, const void *const *params, void *packed, void *stream);

/* ---- model level  (model/waveglow.py:150-208, model/base.py:20-55) ------------------------- */
/* WaveGlow.forward_computation (waveglow.py:150-179): audio[B,N], h[B,n_mels,F] -> z[B,N], logdet[B]. */
int wg_forward(const wg_config *cfg, const void *packed, const float *audio, const float *h,
               int B, int N, int F, float *z, float *logdet, void *ws, size_t ws_bytes, void *stream);

/* WaveGlow.reverse_computation (waveglow.py:181-208): z[B,N], h -> x[B,N], logdet[B].  FlowBase.infer
 * (base.py:42-55) is this call on a latent the caller draws. */
int wg_inverse(const wg_config *cfg, const void *packed, const float *z, const float *h,
               int B, int N, int F, float *x, float *logdet, void *ws, size_t ws_bytes, void *stream);

/* Backward of wg_forward with the reference's constant-memory protocol (efficient_modules.py:118-154,
 * 230-244): starts from the flow OUTPUT z, walks flows last to first, rebuilds each block's input from
 * its output, recomputes that flow's WN activations into the workspace and produces the gradient of every
 * parameter.  dz[B,N], dlogdet[B] are the incoming gradients.  grads: table as params (written, not
 * accumulated).  dh[B,n_mels,F] and dx[B,N] (gradient wrt the audio) may be NULL.  x_rebuilt (nullable)
 * receives the re-materialised input audio [B,N].
 * flow_events (nullable): n_flows+1 caller-created hipEvent_t; [k] is recorded on `stream` as soon as every parameter
 * gradient of flow k (its WN and its 1x1 weight) is final, [n_flows] after the upsampler's -- lets a data-parallel caller
 * all-reduce one flow's bucket over RCCL while the remaining flows are still in backward (what DDP's bucket hooks do
 * for the reference, train.py:77). */
int wg_backward(const wg_config *cfg, const void *const *params, const void *packed,
                const float *z, const float *h, const float *dz, const float *dlogdet,
                int B, int N, int F, void *const *grads, float *dh, float *dx, float *x_rebuilt,
                void *ws, size_t ws_bytes, void *stream, void *const *flow_events);

/* WaveGlowLoss.forward (model/loss.py:10-15): loss = mean_b(0.5*sum z^2/sigma^2 - logdet_b) [/N].
 * loss is a device scalar.  metrics (nullable, 4 device floats) receives the scalars the reference's training step logs
 * next to the loss (model/lightning.py:58-64): [0] logdet.sum() / z.numel(), [1] z.mean(), [2] z.std() (unbiased),
 * [3] the loss -- per process; a data-parallel caller mean-reduces the vector (Lightning's sync_dist=True).
 * scratch: wg_nll_scratch_floats(B) floats.  The backward writes dz[B,N], dlogdet[B] for an upstream gradient dloss
 * (device scalar, NULL = 1). */
size_t wg_nll_scratch_floats(int B);
int wg_nll_loss(const float *z, const float *logdet, int B, int N, float sigma, int elementwise_mean,
                float *loss, float *metrics, float *scratch, void *stream);
int wg_nll_loss_backward(const float *z, int B, int N, float sigma, int elementwise_mean,
                         const float *dloss, float *dz, float *dlogdet, void *stream);

/* ---- block level  (model/efficient_modules.py) ---------------------------------------------- */
/* InvertibleConv1x1.forward_computation / reverse_computation (efficient_modules.py:31-54): W[c,c] device,
 * x[B,c,T] -> z[B,c,T]; logdet = device scalar (+-T*logdet W, NaN when det W < 0 as torch.logdet). */
int wg_invconv_apply(const float *W, int c, const float *x, int B, int T, int reverse,
                     float *z, float *logdet, void *ws, size_t ws_bytes, void *stream);
/* Conv1x1Func.backward / InvConv1x1Func.backward (efficient_modules.py:230-244, 262-279): from the block
 * OUTPUT z and its gradient dz plus dlogdet (device scalar): rebuilt input x, dx, dW[c,c]. */
int wg_invconv_backward(const float *W, int c, const float *z, const float *dz, const float *dlogdet,
                        int B, int T, int reverse, float *x, float *dx, float *dW,
                        void *ws, size_t ws_bytes, void *stream);

/* AffineCouplingBlock.forward_computation / reverse_computation (efficient_modules.py:70-96) with F = WN:
 * x[B,2*in_ch,T], y[B,aux,T] -> z[B,2*in_ch,T], log_s[B,in_ch,T] (negated when reverse). */
int wg_coupling_apply(const wg_wn_dims *d, const void *packed, const float *x, const float *y,
                      int B, int T, int reverse, float *z, float *log_s,
                      void *ws, size_t ws_bytes, void *stream);
/* WN.forward (waveglow.py:98-105): x[B,in_ch,T], y[B,aux,T] -> (log_s, t), each [B,in_ch,T]. */
int wg_wn_apply(const wg_wn_dims *d, const void *packed, const float *x, const float *y, int B, int T,
                float *log_s, float *t, void *ws, size_t ws_bytes, void *stream);
/* NonCausalLayer.forward / NonCausalLayer2D.forward on its own (waveglow.py:18-46, waveflow.py:14-51): xy = W(x) + y; gate = tanh(xy[:Cd]) * sigmoid(xy[Cd:]); o = W_o(gate);
 * returns (o[:C] + x, o[C:]) -- or (none, o) for the last layer.  Any dilation, odd radix <= 9, no bias; exact fp32 MFMA arithmetic.
 * params = {W.weight_g (NULL: plain weight), W.weight_v [2 Cd, C, radix], W_o.weight_g (NULL: plain), W_o.weight_v [C + Cs or Cs, Cd, 1]};
 * x[B,C,T], y[B,2 Cd,T] (the layer's slice of the conditioning projection V(y)) -> res[B,C,T] (NULL when last_layer), skip[B,Cs,T]. */
typedef struct wg_layer_dims {
    int32_t res_ch, dil_ch, skip_ch, radix, dilation, last_layer;
    int32_t h_dilation, rows;   /* NonCausalLayer2D (waveflow.py:14-51): h_dilation > 0 = a radix x radix conv, causal along the height axis
                                 * (dilation h_dilation there); x[B,C,rows,T], y[B,2 Cd,1,T] -> res[B,C,rows,T], skip[B,Cs,rows,T].  0, 0: the 1-D layer */
} wg_layer_dims;
size_t wg_layer_workspace_bytes(const wg_layer_dims *d, int B, int T);
int wg_layer_apply(const wg_layer_dims *d, const void *const *params, const float *x, const float *y, int B, int T,
                   float *res, float *skip, void *ws, size_t ws_bytes, void *stream);
/* What autograd computes upstream for that call (NonCausalLayer / NonCausalLayer2D are ordinary differentiable modules): from d res
 * (NULL: none -- the last layer, or an output nobody used) and d skip, the gradient of x (nullable), of y (nullable; [B,2 Cd,T] -- for the
 * 2-D layer summed over the height axis y was broadcast over) and of the four parameters (`grads`: the layout of `params`; entries of a
 * plain weight's g and entries nobody needs are NULL).  Workspace: wg_layer_backward_workspace_bytes. */
size_t wg_layer_backward_workspace_bytes(const wg_layer_dims *d, int B, int T);
int wg_layer_backward(const wg_layer_dims *d, const void *const *params, const float *x, const float *y, const float *dres, const float *dskip,
                      int B, int T, float *dx, float *dy, void *const *grads, void *ws, size_t ws_bytes, void *stream);
/* AffineCouplingFunc.backward / InvAffineCouplingFunc.backward (efficient_modules.py:118-154, 175-212):
 * from the block OUTPUT z, y, dz, dlog_s: rebuilt input x, dx, dy (nullable), parameter grads. */
int wg_coupling_backward(const wg_wn_dims *d, const void *const *params, const void *packed,
                         const float *z, const float *y, const float *dz, const float *dlog_s,
                         int B, int T, int reverse, float *x, float *dx, float *dy, void *const *grads,
                         void *ws, size_t ws_bytes, void *stream);

/* mel upsampler alone (waveglow.py:126-130,210-212, cropped to T as :157): h[B,n_mels,F] -> y[B,n_mels,T] */
int wg_upsample(const wg_config *cfg, const void *packed, const float *h, int B, int F, int T, float *y, void *stream);

/* ---- WSRGlow conditioning front-end -------------------------------------------------------------
 * Replaces WSRGlow._get_cond (model/wsrglow.py:37-50): c[B,L] (low-rate audio, L a multiple of 8) ->
 * cond[B, WG_WSR_COND_CHANNELS, L/8] = cat(mu-law(256) embedding [8*400], |STFT16| [9], phase embedding [9*50]).
 * mu_table is `mu_enc.1.weight` [256,400] (wsrglow.py:27-30), ang_table is `angle_embed.embed.weight` [120,50]
 * (wsrglow.py:8-18,31).  c is read clipped to [-1,1] and NOT modified (the reference clips it in place, wsrglow.py:38:
 * the Python mirror does that).  The result feeds wg_forward / wg_inverse as `h` of a WaveGlow with n_mels = 3659. */
#define WG_WSR_COND_CHANNELS 3659
int wg_wsr_cond(const float *c, int B, int L, const float *mu_table, const float *ang_table, float *cond, void *stream);
/* Diagnostics: the two quantisers' float32 values BEFORE truncation, from the functions wg_wsr_cond truncates: mu_pre[B][L] (the mu-law
 * value (x_mu + 1) / 2 * 255 + 0.5 of every clipped low-rate sample, wsrglow.py:39) and ang_pre[B][9][L/8] ((angle / pi + 1) * 0.5 * 119 of
 * every STFT bin, wsrglow.py:15-18).  A parity test uses them to forgive ONLY decisions that sit within float noise of a bin edge. */
int wg_wsr_cond_pre(const float *c, int B, int L, float *mu_pre, float *ang_pre, void *stream);
/* Its backward: the two nn.Embedding weight gradients from dcond[B,3659,L/8] (c has no gradient path: wsrglow.py:39,48 go
 * through integer indices, :47 has no parameters).  Outputs are overwritten. */
int wg_wsr_cond_backward(const float *c, int B, int L, const float *dcond, float *dmu_table, float *dang_table, void *stream);

/* The training step of model/lightning.py:52-65 in ONE call: forward, WaveGlowLoss(sigma) (loss.py:10-15), backward to every
 * parameter gradient (+ dh when not NULL), and the four logged scalars (metrics, nullable: see wg_nll_loss).  Equivalent to
 * wg_forward + wg_nll_loss + wg_nll_loss_backward + wg_backward; the forward runs in the backward's workspace
 * (wg_workspace_bytes(.., mode 1)) and keeps the layers of the flow it processes last, which the backward then does not
 * recompute.  scratch: wg_train_scratch_floats(B, N) floats.  flow_events as in wg_backward. */
size_t wg_train_scratch_floats(int B, int N);
int wg_train_step(const wg_config *cfg, const void *const *params, const void *packed, const float *audio, const float *h,
                  int B, int N, int F, float sigma, int elementwise_mean, float *z, float *logdet, float *loss, float *metrics,
                  void *const *grads, float *dh, float *scratch, void *ws, size_t ws_bytes, void *stream, void *const *flow_events);

/* ---- WaveFlow (model/waveflow.py) -------------------------------------------------------------------
 * WaveFlow(flows, n_group, n_mels, use_conv1x1=False, ..., dilation/residual/skip_channels, bias=False): audio [B,N] viewed as
 * [B, n_group (height), N/n_group (time)], 8-layer WN2D with 3x3 dilated convs causal along the height axis, autoregressive
 * affine coupling along the height axis, flip between flows.  Parameter table = named_parameters() order (3 + 37 per flow):
 *   upsampler.1.{bias, weight_g, weight_v}; WNs.k.{V.g, V.v, start.g, start.v, layers.i.{W.g, W.v, W_o.g, W_o.v} x 8, end.weight};
 *   with use_conv1x1 followed by invconv1x1.k.weight for every flow (3 + 38 per flow).
 * Every WG_PREC_* arithmetic mode is built for this model (ABI 4).  The hop length is 256 (waveflow.py:160). */
typedef struct wg_wf_config {
    int32_t flows, n_group, n_mels;
    int32_t res_ch, dil_ch, skip_ch;
    int32_t precision;
    int32_t use_conv1x1;    /* WaveFlow(use_conv1x1=True) (waveflow.py:176-181,203-206,224-229): an InvertibleConv1x1(n_group) over the height
                               axis replaces the flip between flows; the parameter table then ends with invconv1x1.{k}.weight [H,H,1] per flow */
    int32_t bias;           /* WN2D(bias=True) (waveflow.py:77,100-122): every conv of every WN2D has a bias.  A flow's part of the table then
                               continues behind end.weight with V.bias, start.bias, 8 x (layers.i.W.bias, layers.i.W_o.bias), end.bias
                               (3 + 56 per flow; the 1x1 weights, when present, still come last) */
} wg_wf_config;
int wg_wf_param_count(const wg_wf_config *cfg);
size_t wg_wf_packed_bytes(const wg_wf_config *cfg);
size_t wg_wf_workspace_bytes(const wg_wf_config *cfg, int B, int N, int mode);      /* 0: forward; 1: backward / inverse */
size_t wg_wf_tape_bytes(const wg_wf_config *cfg, int B, int N);
int wg_wf_pack_weights(const wg_wf_config *cfg, const void *const *params, void *packed, void *stream);
/* WaveFlow._upsample_h (waveflow.py:163-169,255-257): mel[B,n_mels,F] -> y[B,n_mels,T] for T <= F*s - 2*(s/2) + 2*s + 1, s = 256/n_group. */
int wg_wf_upsample(const wg_wf_config *cfg, const void *const *params, const void *packed, const float *mel, int B, int F, int T,
                   float *y, void *stream);
/* WaveFlow.forward_computation (waveflow.py:182-208): z[B,N], logdet[B].  `tape` (nullable; zero-initialised once) receives every
 * flow's input for wg_wf_backward. */
int wg_wf_forward(const wg_wf_config *cfg, const void *const *params, const void *packed, const float *audio, const float *mel,
                  int B, int N, int F, float *z, float *logdet, void *tape, void *ws, size_t ws_bytes, void *stream);
/* WaveFlow.reverse_computation (waveflow.py:210-253): the row-by-row autoregressive inverse. */
int wg_wf_inverse(const wg_wf_config *cfg, const void *const *params, const void *packed, const float *z, const float *mel,
                  int B, int N, int F, float *x, float *logdet, void *ws, size_t ws_bytes, void *stream);
/* WN2D.forward on its own (waveflow.py:128-135): x[B,1,rows,W] with rows <= n_group, y[B,n_mels,W] (already at the flow's time
 * resolution) -> log_s, t, each [B,1,rows,W].  `params` / `packed`: the table and wg_wf_pack_weights of a configuration with flows = 1 whose
 * WN2D entries are this module's parameters (the three upsampler entries are packed but not read here). */
int wg_wf_wn_apply(const wg_wf_config *cfg, const void *const *params, const void *packed, const float *x, const float *y, int B, int rows, int W,
                   float *log_s, float *t, void *ws, size_t ws_bytes, void *stream);
/* What autograd computes upstream for that call (WN2D is an ordinary differentiable module, waveflow.py:94-135): from the gradients of
 * log_s and t, each [B,1,rows,W], the gradient of x (nullable, [B,1,rows,W]), of y (nullable, [B,n_mels,W]) and of every WN2D parameter
 * (`grads`: the table layout of `params`, null entries skipped; the three upsampler entries are not touched).  Workspace:
 * wg_wf_workspace_bytes(cfg, B, W * n_group, 1). */
int wg_wf_wn_backward(const wg_wf_config *cfg, const void *const *params, const void *packed, const float *x, const float *y,
                      const float *dlog_s, const float *dt, int B, int rows, int W, float *dx, float *dy, void *const *grads,
                      void *ws, size_t ws_bytes, void *stream);
/* What autograd computes upstream for z, logdet = model(x, mel) (the reference trains this model with memory_efficient=False):
 * every parameter gradient (table order), d mel (nullable), d audio (nullable), from the tape wg_wf_forward wrote. */
int wg_wf_backward(const wg_wf_config *cfg, const void *const *params, const void *packed, const void *tape, const float *mel,
                   const float *dz, const float *dlogdet, int B, int N, int F, void *const *grads, float *dmel, float *dx,
                   void *ws, size_t ws_bytes, void *stream);

/* ---- log-mel conditioner ---------------------------------------------------------------------------
 * Replaces MelSpec.forward (model/condition.py:7-19): reflection pad (n_fft/2 - hop/2, n_fft/2 + hop/2), torchaudio
 * MelSpectrogram(sample_rate, n_fft, hop_length, center=False, f_min, f_max, n_mels) with torchaudio's defaults for the rest
 * (periodic Hann, power 2, HTK mel scale, norm None), then log(x + 1e-7).  audio[B,N] -> mel[B,n_mels,N/hop + 1].
 * f_max <= 0 means sr // 2.  n_fft must be a power of two <= 2048.  power (nullable, [B, n_fft/2+1, frames]) additionally receives
 * the power spectrogram before the mel filterbank -- the half of the conditioner that is plain torch upstream
 * (nn.ReflectionPad1d + torch.stft(periodic Hann, center=False).abs()**2) and is pinned to torch's own output
 * (tests/golden/cond_melspec_power.npz); the HTK filterbank on top restates torchaudio's published formula.  torchaudio is not part of the reference tree: its published
 * algorithm is restated (parity unpinned against torchaudio itself). */
int wg_melspec_frames(int N, int n_fft, int hop);
int wg_melspec(const float *audio, int B, int N, int sr, int n_fft, int hop, double f_min, double f_max, int n_mels, float *mel,
               float *power, void *stream);

/* LowPass.forward / STFTDecimate.forward (model/condition.py:22-66), the conditioner of the WSRGlow configs: right zero-pad by
 * n_fft, STFT (center, reflect, periodic Hann), zero the bins >= cut_bins, ISTFT, crop to T, keep every `step`-th sample.
 * STFTDecimate(r) = cut_bins int((n_fft/2+1) / r), step r; LowPass(x, i) = cut_bins int((n_fft/2+1) * ratio[i]), step 1.
 * x[B,T] -> out[B, ceil(T/step)].  ws: wg_lowpass_workspace_bytes. */
size_t wg_lowpass_workspace_bytes(int B, int T, int n_fft, int hop);
int wg_lowpass(const float *x, int B, int T, int n_fft, int hop, int cut_bins, int step, float *out, void *ws, size_t ws_bytes, void *stream);

/* ---- optimizer step (trainer parity) ---------------------------------------------------------------
 * torch.optim.Adam (amsgrad = false, maximize = false) on one contiguous fp32 range: what the reference's
 * configure_optimizers builds from `optimizer` in its configs (model/lightning.py:41-44; configs/waveglow_LJ_speech.json:
 * lr 1e-4; configs/wsrglow_vctk_2x.json: betas (0.9, 0.98)).  `step` is 1-based.  All four ranges must be 16-byte aligned.
 * Hyper-parameters are doubles (Python floats upstream): 1 - beta is formed in double before it is rounded to fp32. */
int wg_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, int step, void *stream);

/* The affine coupling by itself, on plain arrays of n = B * ic * T floats: what AffineCouplingBlock computes around a transform that is
 * NOT this library's WN (efficient_modules.py:58-62 accepts any `transform_type`; the transform then runs as the caller's module).
 * apply: out = in * exp(log_s) + t, or (reverse) (in - t) / exp(log_s)  (:81 / :94).
 * backward (AffineCouplingFunc.backward :132-148 / InvAffineCouplingFunc.backward :194-206): from the block output's second half, the
 * recomputed log_s and t, the gradient of that half and of the returned log_s (nullable): the block input's second half rebuilt, the
 * gradients w.r.t. the transform's outputs (g_log_s, g_t: the seeds of its backward) and the gradient of the input half. */
int wg_affine_apply(const float *in, const float *log_s, const float *t, size_t n, int reverse, float *out, void *stream);
int wg_affine_backward(const float *out_half, const float *log_s, const float *t, const float *dout, const float *dlog_s, size_t n, int reverse,
                       float *in_rebuilt, float *g_log_s, float *g_t, float *din, void *stream);

/* ---- MelGlow (model/melglow.py upstream): the location-variable-convolution WN and its kernel predictor ---------------------
 * Appended to revision 9 without changing any earlier declaration (revision 10: the BatchNorm statistics in double).  Building
 * blocks, each one launch (or a few) on the caller's
 * stream; the composition (Predictor, NonCausalLayerLVC, WN_LVC) is driven from melglow.py.  Exact fp32 (fma chains on the vector
 * ALUs): the result does not depend on WG_PREC_*.  None of them needs a workspace: every buffer is an argument.  Every reduction
 * has a fixed order (no atomics), so a recompute reproduces its forward bit for bit. */

/* C[b] = alpha * op(A)[b] op(B)[b] + beta * D[b] (D nullable: then the beta term is absent; D may alias C) with element strides:
 *   A[m][k] at a_b*b + a_m*m + a_k*(k % K1) + a_k2*(k / K1)
 *   B[k][n] at b_b*b + b_k*(k % K1) + b_k2*(k / K1) + b_n*(n % N1) + b_n2*(n / N1)
 *   C[m][n] at c_b*b + c_m*m + c_n*(n % N1) + c_n2*(n / N1)          (D: the same offsets)
 * The two-level N / K axes read a [B, C, F] tensor as [C, B * F] columns, or sum a weight gradient over items and positions.
 * A product with few output tiles and a long K (a weight gradient) is cut along K into slices whose partial sums go to the
 * workspace and are added in slice order (deterministic); ws: wg_mg_gemm_workspace_bytes(d) bytes (0: none needed, ws may be NULL). */
typedef struct wg_mg_gemm_desc {
    int32_t M, N, K, batch;
    int32_t N1, K1;
    int64_t a_m, a_k, a_k2, a_b;
    int64_t b_k, b_k2, b_n, b_n2, b_b;
    int64_t c_m, c_n, c_n2, c_b;
    float alpha, beta;
} wg_mg_gemm_desc;
size_t wg_mg_gemm_workspace_bytes(const wg_mg_gemm_desc *d);
int wg_mg_gemm(const wg_mg_gemm_desc *d, const float *A, const float *B, const float *D, float *C, void *ws, size_t ws_bytes,
               void *stream);

/* BatchNorm1d over rows of x[C][N] (N = B * frames).  stats: train = 1 -> batch mean, 1/sqrt(biased var + eps) and the unbiased
 * variance (sums in double, fixed order); train = 0 -> the same three from running_mean / running_var.  mean and invstd are
 * double[C]: tanh and tanh_backward subtract the mean from x in double, so a mean that is large against the deviation costs no
 * accuracy, and the backward's dyh - mean(dyh) - xh mean(dyh xh), which cancels to order eps when a channel has two values, is
 * formed in double.
 * update: running = momentum * batch + (1 - momentum) * running (the unbiased variance for running_var), ++*num_batches_tracked
 * (nullable) -- a launch of its own, so that the caller decides when the running statistics move.
 * tanh: s = tanh((x - mean) * invstd * gamma + beta), sum = s + res (res nullable; gamma / beta nullable = affine off).
 * tanh_backward: from ds (gradient of s): dx with batch statistics (train = 1) or constants (train = 0), dgamma / dbeta (nullable). */
int wg_mg_bn_stats(const float *x, int C, int N, float eps, int train, const float *running_mean, const float *running_var, double *mean,
                   double *invstd, float *var_unbiased, void *stream);
int wg_mg_bn_update(float *running_mean, float *running_var, int64_t *num_batches_tracked, const double *mean, const float *var_unbiased,
                    int C, float momentum, void *stream);
int wg_mg_bn_tanh(const float *x, int C, int N, const double *mean, const double *invstd, const float *gamma, const float *beta,
                  const float *res, float *s, float *sum, void *stream);
int wg_mg_bn_tanh_backward(const float *ds, const float *s, const float *x, int C, int N, const double *mean, const double *invstd,
                           const float *gamma, int train, float *dx, float *dgamma, float *dbeta, void *stream);

/* weight norm over dim 0 of a [rows][cols] weight: w = g v / ||v||, and its backward (dg nullable). */
int wg_mg_weight_norm(const float *g, const float *v, int rows, int cols, float *w, void *stream);
int wg_mg_weight_norm_backward(const float *g, const float *v, const float *dw, int rows, int cols, float *dg, float *dv, void *stream);

/* NonCausalLayerLVC's dilated conv (model/melglow.py:75-90): x[B][R][T], T = F * L (L columns per frame), per-frame kernels
 * w[B][F][2D][R][radix] (each frame's block contiguous), padding dilation * (radix - 1) / 2 on both sides of the whole signal:
 *   z[b][o][fL + t] = sum_{ci,k} w[b][f][o][ci][k] x[b][ci][fL + t + (k - radix/2) dilation]   (zero outside [0, T))
 *   gate = tanh(z[:, :D]) * sigmoid(z[:, D:])                                                 (fused_gate, waveglow.py:13-15)
 * backward_data: dx = dx_add (nullable; may alias dx) + the transpose of that map, summed over the overlapping frame windows
 * by gathering (no atomics).  backward_weight: dw[b][f] = dz over the frame's columns times the unfolded window.
 * gate_backward: dz[B][2D][T] from z and the gate's gradient dgate[B][D][T].
 * check: WG_OK, or why the kernels do not serve the shape: even radix (WG_EUNSUPPORTED), T % F (WG_ESHAPE), D > 128, R > 128,
 * R * radix > 256, L > 128, D * L or R * L > 2048 (WG_EUNSUPPORTED).  The launching entry points run the same check first. */
typedef struct wg_lvc_dims {
    int32_t res_ch, dil_ch, radix, dilation;
} wg_lvc_dims;
int wg_lvc_check(const wg_lvc_dims *d, int B, int T, int F);
int wg_lvc_forward(const wg_lvc_dims *d, const float *x, const float *w, int B, int T, int F, float *z, float *gate, void *stream);
int wg_lvc_backward_data(const wg_lvc_dims *d, const float *dz, const float *w, const float *dx_add, int B, int T, int F, float *dx,
                         void *stream);
int wg_lvc_backward_weight(const wg_lvc_dims *d, const float *dz, const float *x, int B, int T, int F, float *dw, void *stream);
int wg_lvc_gate_backward(const float *z, const float *dgate, int B, int D, int T, float *dz, void *stream);

/* ---- MRWaveGlow (model/mr_waveglow.py upstream): the multi-resolution plumbing around its couplings --------------------------
 * Appended to revision 10 without changing any earlier declaration (purely additive: the revision stays 10).  The couplings
 * themselves are wg_coupling_* / wg_invconv_*; these six launches are what is left: exact fp32, no workspace, no atomics, the same
 * bits in every WG_PREC_* mode and on every run.  Every one checks its arguments first and launches nothing when it returns an error.
 *
 * haar_split: x[b][ch][t] at x + s_b*b + s_c*ch + s_t*t (element strides >= 0, so level 0 reads the audio's [B, T, n_group] layout
 *   as it is), c even: diff[b][i][t] = a (x[2i+1] - x[2i]), avg[b][i][t] = b (x[2i] + x[2i+1]), both [B][c/2][T] contiguous, and
 *   (cond nullable) the same avg into rows [0, c/2) of cond[B][cond_rows][T].  mode 0: (a, b) = (1, 1/2), a level of the forward pass
 *   (mr_waveglow.py:73-74); mode 1: (1/2, 1), the backward of haar_merge (davg = dz0 + dz1, ddiff = (dz1 - dz0) / 2).
 * haar_merge: out[b][2i][t] = a m - b diff, out[b][2i+1][t] = a m + b diff with m = avg (+ avg2[b][i][t] of [B][avg2_rows][T],
 *   nullable), out by element strides (o_c, o_t >= 1).  mode 0: (1, 1/2), the merge of the reverse pass (:126-127); mode 1: (1/2, 1), the backward of
 *   haar_split (dx0 = davg / 2 - ddiff, dx1 = davg / 2 + ddiff; avg2 = the rows of the conditioning buffer's gradient).
 * upsample: F.interpolate(h[B][n_mels][F], scale_factor = s, mode = 'linear') (:133-134, align_corners false) cut to its first T
 *   columns (T <= F s, else WG_ESHAPE), into rows [r0, r0 + n_mels) of out[B][rows][T]; head (nullable, [B][r0][T]) is copied to rows
 *   [0, r0) by the same launch, which makes out = cat([head, y], 1).  Column t reads position (2t + 1 - s) / (2s): below 0 it is frame
 *   0, else frames i0 = p / 2s and min(i0 + 1, F - 1) with weights from the integer remainder (a clamped pair is the frame itself).
 * upsample_backward: dh[B][n_mels][F] from rows [r0, r0 + n_mels) of dout[B][rows][T]: every frame sums, in column order, the at
 *   most 2s columns that read it (0 for a frame past the cut).
 * pack / unpack: src[B][c][T] -> dst[b][t][off + ch] of the latent [B][T][n_group] (mr_waveglow.py:93), and back (:98-106). */
int wg_mr_haar_split(const float *x, int64_t s_b, int64_t s_c, int64_t s_t, int B, int c, int T, int mode, float *diff, float *avg,
                     float *cond, int cond_rows, void *stream);
int wg_mr_haar_merge(const float *avg, const float *avg2, int avg2_rows, const float *diff, int B, int c, int T, int mode, float *out,
                     int64_t o_b, int64_t o_c, int64_t o_t, void *stream);
int wg_mr_upsample(const float *h, const float *head, int B, int n_mels, int F, int s, int T, float *out, int rows, int r0, void *stream);
int wg_mr_upsample_backward(const float *dout, int rows, int r0, int B, int n_mels, int F, int s, int T, float *dh, void *stream);
int wg_mr_pack(const float *src, int B, int c, int T, int n_group, int off, float *dst, void *stream);
int wg_mr_unpack(const float *src, int B, int c, int T, int n_group, int off, float *dst, void *stream);

/* ---- MelGlow, model level: the eval-mode passes (model/melglow.py:196-258 upstream with every module in eval()) ------------------
 * Appended to revision 10 without changing any earlier declaration (purely additive: the revision stays 10).  What wg_forward /
 * wg_inverse are to WaveGlow: MelGlow.forward_computation / reverse_computation as ONE call each, from weights packed once per
 * weight change and one workspace.  No autograd counterpart: the training step stays composed from the building blocks above.
 * Exact fp32 on the vector ALUs (the result does not depend on WG_PREC_*), every reduction in a fixed order: two runs give the same bits.
 *
 * wg_mg_config: the arguments of MelGlow(...) and the WN_LVC keyword arguments it forwards.  A frame owns L = hop / n_group columns.
 * reverse_mode: MelGlow(reverse_mode=True) builds every block with the switch set (base.py:20-28), so forward_computation then walks the
 * flows first to last with each block's z -> x arithmetic and reverse_computation last to first with the x -> z arithmetic.
 *
 * Table ("table" of wg_mg_pack_weights): device pointers in the order of the model's state_dict() restricted to its float tensors
 * (parameters and BatchNorm running_mean / running_var; num_batches_tracked is skipped), wg_mg_param_count entries:
 *     [0 .. flows)                  invconv1x1.{k}.weight [c_k, c_k, 1]
 *     then per flow k (WNs.{k}.F.), 9 + 2 depth + 10 pred_layers entries:
 *         start.weight_g, start.weight_v [res_ch, c_k / 2, 1]
 *         layers.{i}.W_o.weight_g, layers.{i}.W_o.weight_v [res_ch + skip_ch (skip_ch in the last layer), dil_ch, 1]   (i = 0 .. depth-1)
 *         end.weight [c_k, skip_ch, 1]
 *         pred.start.0.weight [H G, n_mels, 1], pred.start.1.{weight, bias, running_mean, running_var} [H G]   (H = pred_ch, G = depth)
 *         pred.end.weight [2 dil_ch res_ch radix G, H, 1]
 *         pred.res_blocks.{r}.0.weight [H G, H, 1], .1.{weight, bias, running_mean, running_var},
 *         pred.res_blocks.{r}.3.weight [H G, H, 1], .4.{weight, bias, running_mean, running_var}                      (r = 0 .. pred_layers-1)
 * A NULL weight_g means the conv carries a plain weight in its weight_v slot (as `params` of wg_layer_apply); nothing else may be NULL.
 * bn_eps (host, nullable = 1e-5 everywhere): flows x (1 + 2 pred_layers) values, the eps of every BatchNorm in table order.
 *
 * pack_weights (once per weight change, not per call): the weight-normed start and W_o, every BatchNorm's running mean and
 * 1 / sqrt(var + eps) as double[C] (what wg_mg_bn_stats(train = 0) produces) next to its weight / bias, and per 1x1 what
 * wg_invconv_apply needs in both directions: W, W^-1, log|det W| (NaN for a negative determinant).
 *
 * forward / inverse: audio (z) [B, N] read as [B, T, n_group], N % hop == 0 or WG_ESHAPE; h [B, n_mels, F] with F >= N / hop, only its
 * first N / hop frames read (through the stride F); early outputs leave and re-enter at the channel offsets of z_split_sizes;
 * logdet[B] = sum over flows of (+-) T log|det W| + the per-item sum of log_s.  The input is not modified.  Everything is enqueued on
 * `stream` in one linear chain: no allocation, no synchronisation, no read-back, so the call can be captured into a graph.
 *
 * check: WG_OK, or why the passes do not serve the shape, before anything is launched: everything outside wg_lvc_check's limits for
 * the layers' dilations 1 .. 2^(depth-1), more than 64 flows, depth > 16, n_group > 32, a flow with an odd number of channels, hop not a
 * multiple of n_group, skip_ch or pred_ch > 4096, n_mels > 65536, pred_layers > 64, B * (N / hop) > 65535 * 64, n_mels * F or B * N
 * past 2^31 - 1 (WG_EUNSUPPORTED); N % hop or F < N / hop (WG_ESHAPE).
 * workspace_bytes / packed_bytes / param_count return 0 for a configuration (or shape) the check refuses. */
typedef struct wg_mg_config {
    int32_t flows, n_group, n_early_every, n_early_size, hop, n_mels;
    int32_t depth, res_ch, dil_ch, skip_ch, radix, pred_ch, pred_layers;
    int32_t reverse_mode;
} wg_mg_config;
int    wg_mg_check(const wg_mg_config *cfg, int B, int N, int F);
int    wg_mg_param_count(const wg_mg_config *cfg);
size_t wg_mg_packed_bytes(const wg_mg_config *cfg);
size_t wg_mg_workspace_bytes(const wg_mg_config *cfg, int B, int N);
int    wg_mg_pack_weights(const wg_mg_config *cfg, const void *const *table, const float *bn_eps, void *packed, void *stream);
int    wg_mg_forward(const wg_mg_config *cfg, const void *packed, const float *audio, const float *h, int B, int N, int F,
                     float *z, float *logdet, void *ws, size_t ws_bytes, void *stream);
int    wg_mg_inverse(const wg_mg_config *cfg, const void *packed, const float *z, const float *h, int B, int N, int F,
                     float *x, float *logdet, void *ws, size_t ws_bytes, void *stream);
/* diagnostics, like the other wg_stat_*: passes run by this process, and launches of the one-launch layer kernel (lvc_layer_kernel:
 * flows x depth per pass) */
long long wg_stat_mg_pass_calls(void);
long long wg_stat_mg_layer_launches(void);
/* The two pieces of a pass on their own (what the tests measure them through).
 * layer_apply: one NonCausalLayerLVC in one launch: h [B][res_ch][T], w [B][F][2 dil_ch][res_ch][radix] as wg_lvc_forward, wo the effective
 *   W_o [res_ch + skip_ch (skip_ch when last)][dil_ch] -> h_next = h + res (a buffer other than h: neighbouring frames read h as their
 *   halo; not written when last) and skip [B][skip_ch][T], stored when first, else added to in place.  Limits: wg_lvc_check.
 * predictor_apply: Predictor.forward in eval() for flow `flow` of a packed model: h [B][n_mels][F], its first Fr frames ->
 *   kernels [depth][B Fr][2 dil_ch res_ch radix] (each frame's kernel contiguous).  ws: 3 planes of pred_ch depth B Fr floats, each
 *   rounded up to a multiple of 4 floats. */
int    wg_mg_layer_apply(const wg_lvc_dims *d, int skip_ch, int first, int last, const float *h, const float *w, const float *wo,
                         int B, int T, int F, float *h_next, float *skip, void *stream);
int    wg_mg_predictor_apply(const wg_mg_config *cfg, const void *packed, int flow, const float *h, int B, int Fr, int F, float *kernels,
                             void *ws, size_t ws_bytes, void *stream);

/* ---- MRWaveGlow, model level: the eval-mode passes (model/mr_waveglow.py:56-136 upstream) ---------------------------------------
 * Appended to revision 10 without changing any earlier declaration (purely additive: the revision stays 10).  What wg_forward /
 * wg_inverse are to WaveGlow: MRWaveGlow.forward_computation / reverse_computation as ONE call each, from weights packed once per
 * weight change and one zero-initialised workspace (wg_workspace_init once; the passes keep every halo and padding row zero).  The WNs
 * and the 1x1 mixes are the kernels wg_forward runs, in the arithmetic `precision` names (WG_PREC_*); the Haar splits and merges and
 * the upsampling are exact fp32 with the values of wg_mr_haar_split / merge / upsample, written straight into the engine's planes.
 * No autograd counterpart: the training step stays composed from the blocks.
 *
 * wg_mr_config: the arguments of MRWaveGlow(...) and the WN keyword arguments it forwards.  levels - 1 levels of `flows` flows each on
 * the Haar differences (c_l = n_group / 2^(l+1) channels, conditioned on the level's average stacked on the upsampled mel, or on the
 * average alone with super_resolution), then prior_flows flows on the last average, conditioned on the upsampled mel.  reverse_mode:
 * the couplings and the PRIOR 1x1 convs swap their two directions, the level 1x1 convs never do (upstream builds them as
 * InvertibleConv1x1(c, c), whose second argument is memory_efficient): in such a model a pass applies W^-1 at the levels where it
 * applies W in the prior, and the sign of T log|det W| in logdet is per flow.
 *
 * Table ("table" of wg_mr_pack_weights): device pointers in the order of the model's state_dict(), wg_mr_param_count entries:
 *     prior_invconv1x1.{k}.weight [c, c, 1]                          (k = 0 .. prior_flows-1)
 *     prior_WNs.{k}.F.*             one WN each, see below
 *     invconv1x1_list.{l}.{k}.weight [c_l, c_l, 1]                   (l = 0 .. levels-2, k = 0 .. flows-1)
 *     WNs_list.{l}.{k}.F.*
 * A WN is V, start, (layers.{i}.W, layers.{i}.W_o) x depth as (weight_g, weight_v) pairs, then end.weight: 4 + 4 depth + 1 entries;
 * with bias every conv's bias stands in front of its pair and end.bias behind end.weight (the state dict's order), + 2 + 2 depth + 1.
 * A NULL weight_g means the conv carries a plain weight in its weight_v slot (weight norm removed); nothing else may be NULL.
 *
 * pack_weights (once per weight change, not per call): every WN as wg_wn_pack_weights packs it at the block's own (in_ch, aux_ch), and
 * per 1x1 what wg_invconv_apply forms per call: W, W^-1, log|det W| (NaN for a negative determinant).
 *
 * forward / inverse: audio (z) [B, N] read as [B, T, n_group], h [B, n_mels, F] with T <= F (hop_size / n_group); the latent holds the
 * levels' differences and the prior's average at the channel offsets of z_split_sizes.  logdet[B] = sum over flows of (+-) T log|det W|
 * + the per-item sum of log_s, summed in a fixed order: two runs give the same bits.  The inputs are only read.  Everything is enqueued on
 * `stream` in one linear chain: no allocation, no synchronisation, no read-back, so the call can be captured into a graph.
 *
 * check: WG_OK, or why the passes do not serve the call, before anything is launched (it needs no device): what MRWaveGlow's
 * constructor refuses -- n_group no multiple of 2^levels, hop_size < n_group --, a precision outside WG_PREC_* and a depth outside
 * 1 .. 16 (WG_EINVAL);
 * n_group > 32, no flow at all (prior_flows = 0 with flows = 0 or levels = 1) or more than 64, and whatever the WN kernels refuse for one
 * of the (in_ch, aux_ch) pairs: channels no multiple of 32, an even or > 9 radix (WG_EUNSUPPORTED); N % n_group or
 * T > F (hop_size / n_group) (WG_ESHAPE); B > 65535 or B N past 2^31 - 1 (WG_EUNSUPPORTED).
 * workspace_bytes / packed_bytes / param_count return 0 for a configuration (or shape) the check refuses. */
typedef struct wg_mr_config {
    int32_t prior_flows, flows, levels, n_group, hop_size, n_mels, super_resolution, reverse_mode;
    int32_t dilation_channels, residual_channels, skip_channels, depth, radix, bias;
    int32_t precision;
} wg_mr_config;
int    wg_mr_check(const wg_mr_config *cfg, int B, int N, int F);
int    wg_mr_param_count(const wg_mr_config *cfg);
size_t wg_mr_packed_bytes(const wg_mr_config *cfg);
size_t wg_mr_workspace_bytes(const wg_mr_config *cfg, int B, int N);
int    wg_mr_pack_weights(const wg_mr_config *cfg, const void *const *table, void *packed, void *stream);
int    wg_mr_forward(const wg_mr_config *cfg, const void *packed, const float *audio, const float *h, int B, int N, int F,
                     float *z, float *logdet, void *ws, size_t ws_bytes, void *stream);
int    wg_mr_inverse(const wg_mr_config *cfg, const void *packed, const float *z, const float *h, int B, int N, int F,
                     float *x, float *logdet, void *ws, size_t ws_bytes, void *stream);
/* diagnostics, like the other wg_stat_*: passes run by this process */
long long wg_stat_mr_pass_calls(void);
/* The passes' plane kernels on their own, through the passes' launch helpers (what the tests measure them through).  A plane is
 * [B][rows][P] floats, P = H + roundup(T, 128) + H, column t of a row at H + t (plane_geo gives H and P for T columns and a halo of at
 * least `halo`); a kernel writes columns [0, T) of the rows it owns and nothing else.
 * plane_split: the c channels of `audio` [B, T c] read as [B, T, c], or rows [0, c) of the plane `src` (exactly one of the two) ->
 *   diff = x1 - x0 into rows [diff_ch0, + c/2) of `diff`, avg = (x0 + x1) / 2 into rows [0, c/2) of `cond` and (nullable) rows
 *   [avg_ch0, + c/2) of `avg`.
 * plane_merge: rows [0, c/2) of `avg` and rows [diff_ch0, + c/2) of `diff` -> avg -+ diff / 2 at rows (2i, 2i + 1) of the plane `out`, or
 *   into `audio` [B, T c] as [B, T, c] (exactly one of the two).
 * plane_upsample: wg_mr_upsample's values into rows [ch0[j], + n_mels) of each of the nd <= 7 planes, formed once. */
int    wg_mr_plane_geo(int T, int halo, int *H, int *P);
int    wg_mr_plane_split(const float *audio, const float *src, int src_rows, int B, int T, int halo, int c, float *diff, int diff_rows,
                         int diff_ch0, float *cond, int cond_rows, float *avg, int avg_rows, int avg_ch0, void *stream);
int    wg_mr_plane_merge(const float *avg, int avg_rows, const float *diff, int diff_rows, int diff_ch0, int B, int T, int halo, int c,
                         float *out, int out_rows, float *audio, void *stream);
int    wg_mr_plane_upsample(const float *h, int B, int n_mels, int F, int s, int T, int halo, int nd, float *const *planes, const int *rows,
                            const int *ch0, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WGFLOW_H */
