"""MelGlow on the HIP kernels of csrc/wg_lvc.h: same constructors, module tree (state-dict names and shapes) and forward / reverse /
infer contract as the reference's model/melglow.py.

    Predictor          start = [Conv1d(aux -> H G, 1), BatchNorm1d, Tanh]; res_blocks.{r} = [grouped 1x1, BN, Tanh] x 2 plus the
                       identity; end = grouped 1x1 (H G -> M G, groups G), M = 2 D R radix: one conv kernel per (item, frame, layer)
    NonCausalLayerLVC  the dilated conv of a layer with those per-frame kernels, fused_gate, W_o (weight norm)
    WN_LVC             start (weight norm) -> layers -> end, (log_s, t) = the two halves of end's output
    MelGlow            WaveGlow's flow stack (InvertibleConv1x1 + AffineCouplingBlock(WN_LVC)) on the mel frames as they are

Every product, BatchNorm, gate and weight norm is a HIP launch (wg_mg_* / wg_lvc_*); torch only owns the tensors.  WN_LVC does not
define `hip_dims`, so AffineCouplingBlock runs it through its generic path: no graph kept in forward, the transform recomputed in
backward -- and with it the reference's BatchNorm semantics: in train() every call of the transform moves the running statistics
(twice per step when memory-efficient, once otherwise; also in `infer`, which does not switch to eval()).

In eval() with autograd disabled a whole pass is ONE library call instead (MelGlow._engine_pass: wg_mg_forward / wg_mg_inverse from
packed weights, csrc/wg_mgflow.h); everything else -- train(), grad enabled, the modules on their own -- stays on the path above.

Layout.  The predictor's activations are [channels, B * frames] (column n = b F + f), read from and written to the callers' [B, C, F]
tensors by the products' strides.  Inside WN_LVC the predicted kernels are [depth][B * F][2D R radix] (each frame's kernel contiguous,
what the LVC kernels read); the stand-alone Predictor returns the reference's [B, depth * M, F].
"""
import os
import weakref
from typing import Tuple

import torch
from torch import Tensor, nn
from torch.autograd import Function

from . import engine
from ._lib import WgError, WgLvcDims, WgMgConfig
from .base import FlowBase
from .efficient_modules import AffineCouplingBlock, InvertibleConv1x1
from .utils import SlotTable, add_weight_norms, conv_gv, conv_gv_slots

__all__ = ["Predictor", "NonCausalLayerLVC", "WN_LVC", "MelGlow"]


# ---- shared pieces ---------------------------------------------------------------------------------------------------------------
def _device_check(*tensors):
    engine.require_device(*tensors)


def _conv_weight(conv):
    """(effective [rows, cols] weight, g, v) of a 1x1 conv: weight norm finalised by wg_mg_weight_norm, or the plain weight."""
    g, v = conv_gv(conv)
    if g is None:
        return v.detach().reshape(v.size(0), -1), None, v
    return engine.mg_weight_norm(g.detach(), v.detach()), g, v


def _conv_grads(conv_w, dw, grads):
    """grads[id(param)] for a conv whose effective weight got gradient dw ([rows, cols])."""
    _, g, v = conv_w
    if g is None:
        grads[id(v)] = dw.view_as(v)
    else:
        dg, dv = engine.mg_weight_norm_backward(g.detach(), v.detach(), dw.view_as(v))
        grads[id(g)], grads[id(v)] = dg, dv


def _no_bias(*convs):
    for c in convs:
        if c.bias is not None:
            raise WgError("MelGlow with bias=True is not built in the HIP kernels (wg_lvc.h): construct it with bias=False")


def _bn_forward(bn, a):
    """BatchNorm1d's statistics for a [C, N] activation and, in train(), its running-stat update (wg_mg_bn_update)."""
    batch = bn.training or bn.running_mean is None
    if batch and a.size(1) < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % ((a.size(1), a.size(0)),))
    mean, invstd, var_unb = engine.mg_bn_stats(a, bn.eps, batch, bn.running_mean, bn.running_var)
    if bn.training and bn.track_running_stats:
        if bn.momentum is None:                       # cumulative average (BatchNorm's momentum=None)
            momentum = 1.0 / float(bn.num_batches_tracked.item() + 1)
        else:
            momentum = bn.momentum
        engine.mg_bn_update(bn.running_mean, bn.running_var, bn.num_batches_tracked, mean, var_unb, momentum)
    return mean, invstd, batch


def _affine(bn):
    return (None, None) if bn.weight is None else (bn.weight.detach(), bn.bias.detach())


def _bn_backward(bn, stats, ds, s, a, grads):
    mean, invstd, batch = stats
    gamma, _ = _affine(bn)
    dgamma = dbeta = None
    if gamma is not None:
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        grads[id(bn.weight)], grads[id(bn.bias)] = dgamma, dbeta
    return engine.mg_bn_tanh_backward(ds, s, a, mean, invstd, gamma, batch, dgamma, dbeta)


def _pred_layout(G, M, B, F, reference):
    """(s_m, s_g, s_f, s_b): element strides of the predicted kernels, in the reference's [B, G M, F] or the LVC kernels' [G][B F][M]."""
    if reference:
        return F, M * F, 1, G * M * F
    return 1, B * F * M, M, F * M


def _pred_forward(pred, y, reference):
    """Predictor.forward on y [B, aux, F] -> (predicted kernels in the chosen layout, what its backward needs)."""
    B, A, F = y.shape
    N, G = B * F, pred.groups
    H = pred.start[0].out_channels
    w0 = pred.start[0].weight.detach()
    a0 = engine.mg_gemm(w0, y, torch.empty((H, N), dtype=torch.float32, device=y.device), H, N, A,
                        (A, 1, 0, 0), (F, 0, 1, A * F, 0), (N, 1, F, 0), N1=F)
    st0 = _bn_forward(pred.start[1], a0)
    P, _ = engine.mg_bn_tanh(a0, st0[0], st0[1], *_affine(pred.start[1]))
    saved = [(a0, st0, P)]
    for blk in pred.res_blocks:
        a1 = engine.mg_grouped(blk[0].weight.detach().reshape(blk[0].out_channels, -1), P, G)
        st1 = _bn_forward(blk[1], a1)
        s1, _ = engine.mg_bn_tanh(a1, st1[0], st1[1], *_affine(blk[1]))
        a2 = engine.mg_grouped(blk[3].weight.detach().reshape(blk[3].out_channels, -1), s1, G)
        st2 = _bn_forward(blk[4], a2)
        s2, Pn = engine.mg_bn_tanh(a2, st2[0], st2[1], *_affine(blk[4]), res=P)
        saved.append((P, a1, st1, s1, a2, st2, s2))
        P = Pn
    E = pred.end.weight.detach()
    M, Kp = E.size(0) // G, E.size(1)
    s_m, s_g, s_f, s_b = _pred_layout(G, M, B, F, reference)
    out = torch.empty((B, G * M, F) if reference else (G, N, M), dtype=torch.float32, device=y.device)
    engine.mg_gemm(E, P, out, M, N, Kp, (Kp, 1, 0, M * Kp), (N, 0, 1, F, Kp * N), (s_m, s_f, s_b, s_g), batch=G, N1=F)
    return out, (y, saved, P, reference)


def _pred_backward(pred, ctx, dout, need_dy, grads):
    """The predictor's parameter gradients into grads[id(param)]; returns dy (or None)."""
    y, saved, P, reference = ctx
    B, A, F = y.shape
    N, G = B * F, pred.groups
    E = pred.end.weight.detach()
    M, Kp = E.size(0) // G, E.size(1)
    s_m, s_g, s_f, s_b = _pred_layout(G, M, B, F, reference)
    dE = torch.empty_like(E)
    engine.mg_gemm(dout, P, dE, M, Kp, N, (s_m, s_f, s_b, s_g), (1, F, N, 0, Kp * N), (Kp, 1, 0, M * Kp), batch=G, K1=F)
    grads[id(pred.end.weight)] = dE
    dP = engine.mg_gemm(E, dout, torch.empty((G * Kp, N), dtype=torch.float32, device=y.device), Kp, N, M,
                        (1, Kp, 0, M * Kp), (s_m, 0, s_f, s_b, s_g), (N, 1, F, Kp * N), batch=G, N1=F)
    for blk, (Pr, a1, st1, s1, a2, st2, s2) in zip(reversed(pred.res_blocks), reversed(saved[1:])):
        da2 = _bn_backward(blk[4], st2, dP, s2, a2, grads)
        w2 = blk[3].weight.detach().reshape(blk[3].out_channels, -1)
        grads[id(blk[3].weight)] = engine.mg_grouped_wgrad(da2, s1, G, torch.empty_like(blk[3].weight))
        ds1 = engine.mg_grouped(w2, da2, G, transpose=True)
        da1 = _bn_backward(blk[1], st1, ds1, s1, a1, grads)
        w1 = blk[0].weight.detach().reshape(blk[0].out_channels, -1)
        grads[id(blk[0].weight)] = engine.mg_grouped_wgrad(da1, Pr, G, torch.empty_like(blk[0].weight))
        dP = engine.mg_grouped(w1, da1, G, add=dP, transpose=True)
    a0, st0, s0 = saved[0]
    da0 = _bn_backward(pred.start[1], st0, dP, s0, a0, grads)
    H = a0.size(0)
    w0 = pred.start[0].weight.detach()
    dw0 = torch.empty_like(w0)
    engine.mg_gemm(da0, y, dw0, H, A, N, (N, 1, F, 0), (1, A * F, F, 0, 0), (A, 1, 0, 0), K1=F)
    grads[id(pred.start[0].weight)] = dw0
    if not need_dy:
        return None
    dy = torch.empty_like(y)
    engine.mg_gemm(w0, da0, dy, A, N, H, (1, A, 0, 0), (N, 0, 1, F, 0), (F, 1, A * F, 0), N1=F)
    return dy


def _lvc_dims(layer, R, K):
    return WgLvcDims(R, layer.W_o.in_channels, K, layer.dilation)


def _layer_forward(layer, dims, h, w, F, skip, first):
    """One NonCausalLayerLVC: (x + res or None, skip accumulated in place), and what its backward needs."""
    z, gate = engine.lvc_forward(dims, h, w, F)
    wo = _conv_weight(layer.W_o)
    R = dims.res_ch
    last = len(layer.chs_split) == 1
    hn = None if last else engine.mg_conv1x1(wo[0][:R], gate, add=h)
    engine.mg_conv1x1(wo[0][R:] if not last else wo[0], gate, out=skip, add=None if first else skip)
    return hn, (z, gate, wo, last)


def _layer_backward(layer, dims, saved, h, w, F, dres, dskip, grads, dw_out):
    """Gradients of one layer: W_o (weight norm) into grads, the predicted kernels' into dw_out (nullable); returns dh."""
    z, gate, wo, last = saved
    R = dims.res_ch
    W = wo[0]
    dwo = torch.empty_like(W)
    if last:
        dgate = engine.mg_conv1x1(W, dskip, transpose=True)
        engine.mg_conv1x1_wgrad(dskip, gate, dwo)
    else:
        dgate = engine.mg_conv1x1(W[:R], dres, transpose=True)
        dgate = engine.mg_conv1x1(W[R:], dskip, out=dgate, add=dgate, transpose=True)
        engine.mg_conv1x1_wgrad(dres, gate, dwo[:R])
        engine.mg_conv1x1_wgrad(dskip, gate, dwo[R:])
    _conv_grads(wo, dwo, grads)
    dz = engine.lvc_gate_backward(z, dgate)
    if dw_out is not None:
        engine.lvc_backward_weight(dims, dz, h, F, dw_out)
    return engine.lvc_backward_data(dims, dz, w, F, dx_add=dres)


def _grads_for(module, grads):
    return tuple(grads.get(id(p)) for p in module.parameters())


# ---- Predictor ------------------------------------------------------------------------------------------------------------------
class _PredictorFn(Function):
    @staticmethod
    def forward(ctx, y, pred, *params):
        out, saved = _pred_forward(pred, y.detach().contiguous(), reference=True)
        ctx.pred, ctx.saved = pred, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        grads = {}
        dy = _pred_backward(ctx.pred, ctx.saved, dout.contiguous(), ctx.needs_input_grad[0], grads)
        ctx.saved = None
        return (dy, None) + _grads_for(ctx.pred, grads)


class Predictor(nn.Module):
    """The kernel predictor of the LVC layers (melglow.py:13-50 upstream): y [B, in, F] -> [B, groups * out, F]."""

    def __init__(self, in_channels, out_channels, hidden_channels, layers, bias, groups):
        super().__init__()
        self.groups = groups
        width = hidden_channels * groups
        self.start = nn.Sequential(nn.Conv1d(in_channels, width, 1, bias=bias), nn.BatchNorm1d(width), nn.Tanh())
        self.end = nn.Conv1d(width, out_channels * groups, 1, bias=bias, groups=groups)
        self.res_blocks = nn.ModuleList([
            nn.Sequential(nn.Conv1d(width, width, 1, bias=bias, groups=groups), nn.BatchNorm1d(width), nn.Tanh(),
                          nn.Conv1d(width, width, 1, bias=bias, groups=groups), nn.BatchNorm1d(width), nn.Tanh())
            for _ in range(layers)])

    def _check(self, y):
        _no_bias(self.start[0], self.end, *[c for blk in self.res_blocks for c in (blk[0], blk[3])])
        if y.dim() != 3 or y.size(1) != self.start[0].in_channels:
            raise WgError("Predictor expects [B, %d, frames], got %s" % (self.start[0].in_channels, tuple(y.shape)))

    def forward(self, x):
        self._check(x)
        _device_check(x)
        return _PredictorFn.apply(x, self, *self.parameters())


# ---- NonCausalLayerLVC ----------------------------------------------------------------------------------------------------------
class _LayerFn(Function):
    @staticmethod
    def forward(ctx, x, weights, layer, *params):
        B, F = weights.shape[:2]
        dims = _lvc_dims(layer, x.size(1), weights.size(-1))
        x, w = x.detach().contiguous(), weights.detach().contiguous()
        skip = torch.empty((B, layer.chs_split[-1], x.size(2)), dtype=torch.float32, device=x.device)
        hn, saved = _layer_forward(layer, dims, x, w, F, skip, True)
        ctx.layer, ctx.dims, ctx.saved, ctx.F = layer, dims, saved, F
        ctx.save_for_backward(x, w)
        return (skip,) if hn is None else (hn, skip)

    @staticmethod
    def backward(ctx, *douts):
        x, w = ctx.saved_tensors
        layer, dims, saved = ctx.layer, ctx.dims, ctx.saved
        last = saved[3]
        dres = None if last else (torch.zeros_like(x) if douts[0] is None else douts[0].contiguous())
        dskip = douts[-1]
        dskip = torch.zeros((x.size(0), layer.chs_split[-1], x.size(2)), dtype=torch.float32, device=x.device) if dskip is None \
            else dskip.contiguous()
        grads = {}
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        dx = _layer_backward(layer, dims, saved, x, w, ctx.F, dres, dskip, grads, dw)
        return (dx, dw, None) + _grads_for(layer, grads)


class NonCausalLayerLVC(nn.Module):
    """One LVC layer (melglow.py:53-90 upstream): forward(x [B, R, T], weights [B, F, 2D, R, radix]) -> (x + res or None, skip)."""

    def __init__(self, dilation, dilation_channels, residual_channels, skip_channels, radix, bias, last_layer=False):
        super().__init__()
        self.padding = dilation * (radix - 1) // 2
        self.dilation = dilation
        self.chs_split = [skip_channels]
        if last_layer:
            self.W_o = nn.Conv1d(dilation_channels, skip_channels, 1, bias=bias)
        else:
            self.W_o = nn.Conv1d(dilation_channels, residual_channels + skip_channels, 1, bias=bias)
            self.chs_split.insert(0, residual_channels)

    def forward(self, x, weights):
        _no_bias(self.W_o)
        if x.dim() != 3 or weights.dim() != 5 or weights.shape[0] != x.shape[0] or weights.shape[2] != 2 * self.W_o.in_channels \
                or weights.shape[3] != x.shape[1]:
            raise WgError("NonCausalLayerLVC expects x [B, R, T] and weights [B, F, 2D, R, radix], got %s and %s"
                          % (tuple(x.shape), tuple(weights.shape)))
        _check_lvc(_lvc_dims(self, x.size(1), weights.size(-1)), x.size(0), x.size(2), weights.size(1))
        _device_check(x, weights)
        out = _LayerFn.apply(x, weights, self, *self.parameters())
        return (None, out[0]) if len(out) == 1 else out


def _check_lvc(dims, B, T, F):
    rc = engine.lvc_check(dims, B, T, F)
    if rc:
        from ._lib import lib
        why = lib().wg_strerror(rc).decode()
        raise WgError("the LVC kernels do not serve res %d / dil %d channels, radix %d, dilation %d at B %d, T %d, %d frames: %s "
                      "(odd radix, T a multiple of the frames, <= 128 columns per frame, <= 128 channels; include/wgflow.h wg_lvc_check)"
                      % (dims.res_ch, dims.dil_ch, dims.radix, dims.dilation, B, T, F, why))


# ---- WN_LVC ---------------------------------------------------------------------------------------------------------------------
class _WNLVCFn(Function):
    @staticmethod
    def forward(ctx, x, y, wn, *params):
        x, y = x.detach().contiguous(), y.detach().contiguous()
        B, ic, T = x.shape
        F = y.size(2)
        ws = _conv_weight(wn.start)
        h = [engine.mg_conv1x1(ws[0], x)]
        W, psaved = _pred_forward(wn.pred, y, reference=False)
        skip = torch.empty((B, wn.skp_chs, T), dtype=torch.float32, device=x.device)
        lsaved = []
        for l, layer in enumerate(wn.layers):
            hn, s = _layer_forward(layer, wn._dims[l], h[l], W[l], F, skip, l == 0)
            lsaved.append(s)
            if hn is not None:
                h.append(hn)
        we = wn.end.weight.detach().reshape(2 * ic, -1)
        log_s = engine.mg_conv1x1(we[:ic], skip)
        t = engine.mg_conv1x1(we[ic:], skip)
        ctx.wn, ctx.F = wn, F
        ctx.saved = (x, ws, h, W, psaved, skip, lsaved)
        return log_s, t

    @staticmethod
    def backward(ctx, dlog_s, dt):
        wn, F = ctx.wn, ctx.F
        x, ws, h, W, psaved, skip, lsaved = ctx.saved
        ctx.saved = None
        B, ic, T = x.shape
        dlog_s = torch.zeros((B, ic, T), dtype=torch.float32, device=x.device) if dlog_s is None else dlog_s.contiguous()
        dt = torch.zeros((B, ic, T), dtype=torch.float32, device=x.device) if dt is None else dt.contiguous()
        grads = {}
        we = wn.end.weight.detach().reshape(2 * ic, -1)
        dwe = torch.empty_like(wn.end.weight)
        engine.mg_conv1x1_wgrad(dlog_s, skip, dwe.view(2 * ic, -1)[:ic])
        engine.mg_conv1x1_wgrad(dt, skip, dwe.view(2 * ic, -1)[ic:])
        grads[id(wn.end.weight)] = dwe
        dskip = engine.mg_conv1x1(we[:ic], dlog_s, transpose=True)
        dskip = engine.mg_conv1x1(we[ic:], dt, out=dskip, add=dskip, transpose=True)
        dW = torch.empty_like(W)
        dh = None
        for l in range(len(wn.layers) - 1, -1, -1):
            dh = _layer_backward(wn.layers[l], wn._dims[l], lsaved[l], h[l], W[l], F, dh, dskip, grads, dW[l])
        dws = torch.empty_like(ws[0])
        engine.mg_conv1x1_wgrad(dh, x, dws)
        _conv_grads(ws, dws, grads)
        dx = engine.mg_conv1x1(ws[0], dh, transpose=True) if ctx.needs_input_grad[0] else None
        dy = _pred_backward(wn.pred, psaved, dW, ctx.needs_input_grad[1], grads)
        return (dx, dy, None) + _grads_for(wn, grads)


class WN_LVC(nn.Module):
    """The location-variable-convolution WN (melglow.py:93-159 upstream): (log_s, t) = WN_LVC(x [B, in, T], y [B, aux, T / L])."""

    def __init__(self, in_channels, aux_channels, depth, dilation_channels, residual_channels, skip_channels, predict_channels,
                 predict_layers, radix, bias, zero_init=True):
        super().__init__()
        self.dilations = [2 ** i for i in range(depth)]
        self.in_chs = in_channels
        self.res_chs = residual_channels
        self.dil_chs = dilation_channels
        self.skp_chs = skip_channels
        self.rdx = radix
        self.r_field = sum(self.dilations) + 1

        self.start = nn.Conv1d(in_channels, residual_channels, 1, bias=bias)
        self.start.apply(add_weight_norms)
        self.layers = nn.ModuleList(
            NonCausalLayerLVC(d, dilation_channels, residual_channels, skip_channels, radix, bias, last_layer=(i == depth - 1))
            for i, d in enumerate(self.dilations))
        self.layers.apply(add_weight_norms)
        self.end = nn.Conv1d(skip_channels, in_channels * 2, 1, bias=bias)
        if zero_init:
            self.end.weight.data.zero_()
            if bias:
                self.end.bias.data.zero_()
        self.pred = Predictor(aux_channels, 2 * dilation_channels * residual_channels * radix, predict_channels, predict_layers, bias,
                              depth)
        self._dims = [WgLvcDims(residual_channels, dilation_channels, radix, d) for d in self.dilations]

    def _check(self, x, y):
        _no_bias(self.start, self.end, *[m.W_o for m in self.layers])
        self.pred._check(y)
        if x.dim() != 3 or x.size(1) != self.in_chs or y.size(0) != x.size(0):
            raise WgError("WN_LVC expects x [B, %d, T] and y [B, aux, frames], got %s and %s" % (self.in_chs, tuple(x.shape), tuple(y.shape)))
        for d in self._dims:
            _check_lvc(d, x.size(0), x.size(2), y.size(2))

    def forward(self, x, y):
        self._check(x, y)
        _device_check(x, y)
        return _WNLVCFn.apply(x, y, self, *self.parameters())


# ---- MelGlow --------------------------------------------------------------------------------------------------------------------
_ENGINES = weakref.WeakKeyDictionary()      # model -> engine.MelGlowEngine (packed weights, workspaces, graphs): not part of the module's state


class MelGlow(FlowBase):
    """WaveGlow's flow stack with WN_LVC couplings, conditioned on the mel frames without upsampling (melglow.py:162-258 upstream)."""

    def __init__(self, flows, n_group, n_early_every, n_early_size, hop_size, n_mels, memory_efficient, reverse_mode=False, **kwargs):
        super().__init__(hop_size, reverse_mode=reverse_mode)
        self.flows = flows
        self.n_group = n_group
        self.n_early_every = n_early_every
        self.n_early_size = n_early_size
        self.n_mels = n_mels
        self.mem_efficient = memory_efficient
        self.upsample_factor = self._hop_length // n_group

        self.invconv1x1 = nn.ModuleList()
        self.WNs = nn.ModuleList()
        c = n_group
        self.z_split_sizes = []
        for k in range(flows):
            if k and k % n_early_every == 0:              # n_early_size channels leave the flow
                c -= n_early_size
                self.z_split_sizes.append(n_early_size)
            self.invconv1x1.append(InvertibleConv1x1(c, memory_efficient=memory_efficient, reverse_mode=reverse_mode))
            self.WNs.append(AffineCouplingBlock(WN_LVC, memory_efficient=memory_efficient, reverse_mode=reverse_mode,
                                                in_channels=c // 2, aux_channels=n_mels, **kwargs))
        self.z_split_sizes.append(c)
        self._mg_table = SlotTable("mg_slots")

    # -- the one-call eval passes (include/wgflow.h wg_mg_*) ---------------------------------------------------------------------------
    def mg_slots(self):
        """Where every entry of the C ABI's table lives in the module tree: state_dict() order, float tensors only (parameters and
        BatchNorm running statistics), a conv's (weight_g, weight_v) pair as (None, weight) once weight norm was removed."""
        def bn(m):
            return [(m._parameters, "weight"), (m._parameters, "bias"), (m._buffers, "running_mean"), (m._buffers, "running_var")]

        slots = [(m._parameters, "weight") for m in self.invconv1x1]
        for blk in self.WNs:
            wn = blk.F
            slots += list(conv_gv_slots(wn.start))
            for layer in wn.layers:
                slots += list(conv_gv_slots(layer.W_o))
            slots.append((wn.end._parameters, "weight"))
            pred = wn.pred
            slots += [(pred.start[0]._parameters, "weight")] + bn(pred.start[1]) + [(pred.end._parameters, "weight")]
            for rb in pred.res_blocks:
                slots += [(rb[0]._parameters, "weight")] + bn(rb[1]) + [(rb[3]._parameters, "weight")] + bn(rb[4])
        return slots

    def mg_table(self):
        return self._mg_table(self)

    def mg_config(self):
        wn = self.WNs[0].F
        return WgMgConfig(self.flows, self.n_group, self.n_early_every, self.n_early_size, self._hop_length, self.n_mels, len(wn.layers),
                          wn.res_chs, wn.dil_chs, wn.skp_chs, wn.rdx, wn.pred.start[0].out_channels // wn.pred.groups,
                          len(wn.pred.res_blocks), int(self._reverse_mode))

    def mg_engine(self):
        eng = _ENGINES.get(self)
        if eng is None:
            eng = _ENGINES[self] = engine.MelGlowEngine(self.mg_config())
        return eng

    def _engine_route(self, x, h):
        """(None, table, eps) when this call goes through the one-call engine, else (why not, None, None): the module path runs.  The
        engine serves exactly: autograd disabled, every module in eval(), every BatchNorm with running statistics and affine parameters,
        no conv bias, CUDA float32 tensors, a shape wg_mg_check accepts, and WG_MG_ENGINE (read per call) not "0"."""
        if os.environ.get("WG_MG_ENGINE") == "0":
            return "WG_MG_ENGINE=0", None, None
        if torch.is_grad_enabled():
            return "autograd is enabled", None, None
        eps = []
        for m in self.modules():
            if m.training:
                return "a module is in train()", None, None
            if isinstance(m, nn.BatchNorm1d):
                eps.append(m.eps)
            elif isinstance(m, nn.Conv1d) and m.bias is not None:
                return "bias=True", None, None
        if x.dim() != 2 or h.dim() != 3 or x.size(0) != h.size(0) or h.size(1) != self.n_mels:
            return "not audio [B, N] with conditioning [B, n_mels, frames]", None, None
        table = self.mg_table()
        for i, t in enumerate(table):
            if t is None:
                if i < self.flows or (i - self.flows) % (len(table) // self.flows - 1) >= 2 + 2 * len(self.WNs[0].F.layers):
                    return "a BatchNorm without running statistics or affine parameters", None, None
            elif t.dtype != torch.float32:
                return "parameters are not float32", None, None
        N = x.size(1) // self._hop_length * self._hop_length
        rc = self.mg_engine().check(x.size(0), N, h.size(2)) if N else -2
        if rc:
            return "wg_mg_check: code %d" % rc, None, None
        if not (x.is_cuda and x.dtype == torch.float32 and h.dtype == torch.float32 and h.device == x.device and table[0].device == x.device):
            return "tensors are not float32 on one HIP device", None, None
        return None, table, eps

    def _engine_pass(self, x, h, inverse):
        """forward_computation / reverse_computation as one library call (wg_mg_forward / wg_mg_inverse), or None: the module path runs.
        The caller's tensors are only read."""
        why, table, eps = self._engine_route(x, h)
        if why is not None:
            return None
        N = x.size(1) // self._hop_length * self._hop_length
        return self.mg_engine().run(x[:, :N], h, [t.detach() for t in table], eps, inverse, synthesis=inverse != self._reverse_mode)

    def _frames(self, x, h):
        """x [B, N] -> [B, n_group, T] (N cut to whole hops) and the T / upsample_factor mel frames it is conditioned on."""
        if x.dim() != 2 or h.dim() != 3:
            raise WgError("expected audio [B, N] and conditioning [B, n_mels, frames]")
        B = x.size(0)
        x = x[:, :x.shape[1] // self._hop_length * self._hop_length]
        x = x.view(B, -1, self.n_group).transpose(1, 2)
        return x, h[..., :x.shape[2] // self.upsample_factor]

    def forward_computation(self, x: Tensor, h: Tensor) -> Tuple[Tensor, Tensor]:
        out = self._engine_pass(x, h, False)
        if out is not None:
            return out
        B = x.size(0)
        x, y = self._frames(x, h)
        early = []
        sections = [self.n_early_size, self.n_group]
        logdet = 0
        for k, (invconv, coupling) in enumerate(zip(self.invconv1x1, self.WNs)):
            if k and k % self.n_early_every == 0:
                sections[1] -= self.n_early_size
                out, x = x.split(sections, 1)
                early.append(out)
                if self.mem_efficient:
                    x = x.clone()
            x, log_det_W = invconv(x)
            x, log_s = coupling(x, y)
            logdet = logdet + log_det_W + log_s.sum((1, 2))
        early.append(x)
        return torch.cat([o.transpose(1, 2) for o in early], 2).view(B, -1), logdet

    def reverse_computation(self, z: Tensor, h: Tensor) -> Tuple[Tensor, Tensor]:
        out = self._engine_pass(z, h, True)
        if out is not None:
            return out
        B = z.size(0)
        z, y = self._frames(z, h)
        parts = z.split(self.z_split_sizes, 1)
        if self.mem_efficient:
            parts = [p.clone() for p in parts]
        *remained, z = parts
        logdet = 0
        for k, invconv, coupling in zip(range(self.flows - 1, -1, -1), self.invconv1x1[::-1], self.WNs[::-1]):
            z, log_s = coupling.reverse(z, y)
            z, log_det_W = invconv.reverse(z)
            logdet = logdet + log_det_W + log_s.sum((1, 2))
            if k and k % self.n_early_every == 0:
                z = torch.cat((remained.pop(), z), 1)
        return z.transpose(1, 2).contiguous().view(B, -1), logdet
