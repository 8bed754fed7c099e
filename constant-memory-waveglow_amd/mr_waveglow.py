"""MRWaveGlow on the HIP engine: same constructor, module tree (state-dict names and shapes) and forward / reverse / infer contract as
the reference's model/mr_waveglow.py.

    invconv1x1_list.{level}.{k}   InvertibleConv1x1(c_l), c_l = n_group / 2^(level + 1): the flows of the level's Haar difference
    WNs_list.{level}.{k}.F        WN(in = c_l / 2, aux = c_l + n_mels, or c_l when super_resolution): conditioned on the level's Haar
                                  average stacked on the upsampled mel
    prior_invconv1x1.{k}, prior_WNs.{k}.F    the flows of the last average, conditioned on the upsampled mel alone

Every coupling and 1x1 conv is this package's block (wg_coupling_* / wg_invconv_*); what runs around them -- the Haar split and merge,
the linear upsampling of the mel into the conditioning buffers, the packing of the per-level latents -- is csrc/wg_mr.h, one launch
each, wrapped in the autograd Functions below.  Autograd sums what the couplings return for a conditioning buffer; the Functions cut
that sum into the gradient of the average and the gradient of the mel.

Upstream's quirks are kept, because checkpoints and results depend on them:
  * the level 1x1 convs are built as InvertibleConv1x1(c, c): the second positional argument is memory_efficient, so they are always
    memory-efficient and never in reverse mode.  In a reverse_mode=True model they therefore apply W^-1 where the prior ones apply W;
  * the level couplings, the prior couplings and the prior 1x1 convs take both flags.

A memory-efficient block frees the storage of the tensor it is handed.  No block here is ever handed a view of a conditioning buffer or
of the caller's tensors: the split writes the average twice (its own tensor, which the next stage may free, and the rows of the
conditioning buffer, which the couplings keep), level 0 reads the audio through its strides, and the latents are packed by a kernel.
In eval() with autograd disabled a whole pass is ONE library call instead (MRWaveGlow._engine_pass: wg_mr_forward / wg_mr_inverse from
weights packed once per weight change, the state in the engine's planes from the first kernel to the last, the pass towards the audio
replayed from a captured graph under the WG_GRAPHS policy); everything else -- train(), autograd enabled, WG_MR_ENGINE=0, a
configuration wg_mr_check refuses -- is the module path below, unchanged.

With super_resolution upstream hands the very same tensor to the last level's couplings as conditioning and to the first prior 1x1
conv, which frees it and rebuilds it in its backward; here the two are separate tensors with the same values.  Upstream's level
couplings therefore run their backward on a conditioning tensor rebuilt to about 1e-7, these on the original: with super_resolution
the gradients differ from upstream's in the last bits (far inside the 1e-4 bars the fixtures are held to).
"""
import os
import weakref
from typing import Tuple

import torch
from torch import Tensor, nn
from torch.autograd import Function

from . import engine
from ._lib import WgError, WgMrConfig, default_precision
from .base import FlowBase
from .efficient_modules import AffineCouplingBlock, InvertibleConv1x1
from .utils import SlotTable, conv_gv_slots
from .waveglow import WN

_ENGINES = weakref.WeakKeyDictionary()      # model -> engine.MRWaveGlowEngine (packed weights, workspaces, graphs): not part of the module's state

__all__ = ["MRWaveGlow"]


def _or_zeros(g, shape, like):
    return torch.zeros(shape, dtype=torch.float32, device=like.device) if g is None else g.contiguous()


class _LevelSplit(Function):
    """x [B, c, T] (any strides), h [B, n_mels, F] or None -> (x_diff, x_avg, cond): cond = cat([x_avg, upsampled h], 1), or a second
    x_avg without h (mr_waveglow.py:73-78)."""

    @staticmethod
    def forward(ctx, x, h, scale, channels_last):
        x = x.detach()
        B, c, T = x.shape
        half = c // 2
        n_mels = 0 if h is None else h.size(1)
        diff, avg, cond = engine.mr_haar_split(x, 0, half + n_mels)
        if h is not None:
            engine.mr_upsample(h.detach().contiguous(), scale, T, out=cond, r0=half)
        ctx.dims = (B, half, T, n_mels, scale, channels_last, None if h is None else h.size(2))
        return diff, avg, cond

    @staticmethod
    def backward(ctx, ddiff, davg, dcond):
        B, half, T, n_mels, scale, channels_last, F = ctx.dims
        like = next(g for g in (ddiff, davg, dcond) if g is not None)
        dcond = None if dcond is None else dcond.contiguous()
        dx = dh = None
        if ctx.needs_input_grad[0]:
            dx = engine.mr_haar_merge(_or_zeros(davg, (B, half, T), like), _or_zeros(ddiff, (B, half, T), like), 1, channels_last, avg2=dcond)
        if n_mels and ctx.needs_input_grad[1]:
            dh = torch.zeros((B, n_mels, F), dtype=torch.float32, device=like.device) if dcond is None else \
                engine.mr_upsample_backward(dcond, half, n_mels, F, scale)
        return dx, dh, None, None


class _Upsample(Function):
    """h [B, n_mels, F] -> F.interpolate(h, scale_factor=scale, mode='linear')[..., :T]; head [B, r0, T] (or None) is stacked on top:
    cat([head, y], 1) (mr_waveglow.py:96-100, :119)."""

    @staticmethod
    def forward(ctx, h, head, scale, T):
        r0 = 0 if head is None else head.size(1)
        ctx.dims = (r0, h.size(1), h.size(2), scale)
        return engine.mr_upsample(h.detach().contiguous(), scale, T, r0=r0, head=None if head is None else head.detach().contiguous())

    @staticmethod
    def backward(ctx, dout):
        r0, n_mels, F, scale = ctx.dims
        dout = dout.contiguous()
        dh = engine.mr_upsample_backward(dout, r0, n_mels, F, scale) if ctx.needs_input_grad[0] else None
        dhead = dout[:, :r0] if r0 and ctx.needs_input_grad[1] else None
        return dh, dhead, None, None


class _Merge(Function):
    """(z, z_diff) [B, c/2, T] -> z0 = z - z_diff / 2, z1 = z + z_diff / 2 interleaved as channels 2i, 2i + 1 (mr_waveglow.py:126-127);
    channels_last: as a view of a [B, T, c] tensor, which is the audio's layout."""

    @staticmethod
    def forward(ctx, avg, diff, channels_last):
        return engine.mr_haar_merge(avg.detach().contiguous(), diff.detach().contiguous(), 0, channels_last)

    @staticmethod
    def backward(ctx, dz):
        ddiff, davg, _ = engine.mr_haar_split(dz, 1)
        return davg, ddiff, None


class _Pack(Function):
    """per-level [B, c_l, T] tensors -> the latent [B, T * n_group]: cat(., 1).transpose(1, 2).contiguous().view(B, -1) (:93)."""

    @staticmethod
    def forward(ctx, n_group, *parts):
        B, _, T = parts[0].shape
        z = torch.empty((B, T * n_group), dtype=torch.float32, device=parts[0].device)
        off = 0
        for p in parts:
            engine.mr_pack(p.detach().contiguous(), n_group, off, z)
            off += p.size(1)
        ctx.n_group, ctx.sizes = n_group, [p.size(1) for p in parts]
        return z

    @staticmethod
    def backward(ctx, dz):
        dz = dz.contiguous()
        offs = [sum(ctx.sizes[:i]) for i in range(len(ctx.sizes))]
        return (None,) + tuple(engine.mr_unpack(dz, ctx.n_group, o, c) for o, c in zip(offs, ctx.sizes))


class _Unpack(Function):
    """the latent [B, T * n_group] -> its per-level [B, c_l, T] tensors, each in storage of its own (:98-106)."""

    @staticmethod
    def forward(ctx, z, n_group, sizes):
        z = z.detach().contiguous()
        ctx.n_group, ctx.sizes, ctx.shape = n_group, list(sizes), tuple(z.shape)
        offs = [sum(sizes[:i]) for i in range(len(sizes))]
        return tuple(engine.mr_unpack(z, n_group, o, c) for o, c in zip(offs, sizes))

    @staticmethod
    def backward(ctx, *grads):
        like = next(g for g in grads if g is not None)
        B, N = ctx.shape
        dz = torch.empty((B, N), dtype=torch.float32, device=like.device)
        off = 0
        for g, c in zip(grads, ctx.sizes):
            engine.mr_pack(_or_zeros(g, (B, c, N // ctx.n_group), like), ctx.n_group, off, dz)
            off += c
        return dz, None, None


class MRWaveGlow(FlowBase):
    def __init__(self, prior_flows, n_group, hop_size, n_mels, memory_efficient, levels=3, flows=4, super_resolution=False,
                 reverse_mode=False, **kwargs):
        super().__init__(hop_size, reverse_mode)
        self.flows = flows
        self.prior_flows = prior_flows
        self.n_group = n_group
        self.n_mels = n_mels
        self.super_resolution = super_resolution
        self.levels = levels
        self.upsample_factor = hop_size // n_group
        if levels < 1 or n_group % (1 << (levels - 1)) or (n_group >> (levels - 1)) % 2 or self.upsample_factor < 1:
            raise WgError("MRWaveGlow: n_group %d does not split into %d levels of even channel counts (n_group must be a multiple of "
                          "2^levels), or hop_size %d < n_group" % (n_group, levels, hop_size))

        self.prior_invconv1x1 = nn.ModuleList()
        self.prior_WNs = nn.ModuleList()
        self.invconv1x1_list = nn.ModuleList()
        self.WNs_list = nn.ModuleList()

        c = n_group
        self.z_split_sizes = []
        for _ in range(levels - 1):
            c = c // 2
            self.z_split_sizes.append(c)
            # (c, c): the second argument is memory_efficient, as upstream writes it -- always on, never in reverse mode
            self.invconv1x1_list.append(nn.ModuleList([InvertibleConv1x1(c, c) for _ in range(flows)]))
            self.WNs_list.append(nn.ModuleList([
                AffineCouplingBlock(WN, memory_efficient=memory_efficient, reverse_mode=reverse_mode, in_channels=c // 2,
                                    aux_channels=c + (0 if super_resolution else n_mels), **kwargs) for _ in range(flows)]))
        self.z_split_sizes.append(c)
        for _ in range(prior_flows):
            self.prior_invconv1x1.append(InvertibleConv1x1(c, memory_efficient=memory_efficient, reverse_mode=reverse_mode))
            self.prior_WNs.append(AffineCouplingBlock(WN, memory_efficient=memory_efficient, in_channels=c // 2, aux_channels=n_mels,
                                                      reverse_mode=reverse_mode, **kwargs))
        self._mr_table = SlotTable("mr_slots")

    # ---- the one-call engine (wg_mr_forward / wg_mr_inverse) ------------------------------------------------------------------------
    def mr_slots(self):
        """Where every entry of the C ABI's table lives in the module tree: state_dict() order, a conv's (weight_g, weight_v) pair as
        (None, weight) once weight norm was removed."""
        def wn_slots(wn):
            convs = [wn.V, wn.start] + [c for layer in wn.layers for c in (layer.W, layer.W_o)]
            out = []
            for conv in convs:
                out += ([(conv._parameters, "bias")] if wn.has_bias else []) + list(conv_gv_slots(conv))
            return out + [(wn.end._parameters, "weight")] + ([(wn.end._parameters, "bias")] if wn.has_bias else [])

        slots = [(m._parameters, "weight") for m in self.prior_invconv1x1]
        for blk in self.prior_WNs:
            slots += wn_slots(blk.F)
        slots += [(m._parameters, "weight") for level in self.invconv1x1_list for m in level]
        for level in self.WNs_list:
            for blk in level:
                slots += wn_slots(blk.F)
        return slots

    def mr_table(self):
        return self._mr_table(self)

    def mr_config(self, precision=None):
        wn = next((b.F for b in list(self.prior_WNs) + [b for level in self.WNs_list for b in level]), None)
        sizes = (0,) * 6 if wn is None else (wn.dil_chs, wn.res_chs, wn.skp_chs, len(wn.layers), wn.rdx, int(wn.has_bias))
        return WgMrConfig(self.prior_flows, self.flows, self.levels, self.n_group, self._hop_length, self.n_mels, int(self.super_resolution),
                          int(self._reverse_mode), *sizes, default_precision() if precision is None else precision)

    def mr_engine(self):
        """the engine of the arithmetic WG_PRECISION names right now (read per call, as the blocks read it when they are built)"""
        per_model = _ENGINES.get(self)
        if per_model is None:
            per_model = _ENGINES[self] = {}
        prec = default_precision()
        eng = per_model.get(prec)
        if eng is None:
            eng = per_model[prec] = engine.MRWaveGlowEngine(self.mr_config(prec))
        return eng

    def _engine_route(self, x, h):
        """(None, table, key) when this call goes through the one-call engine, else (why not, None, None): the module path runs.  The
        engine serves exactly: autograd disabled, the model in eval(), CUDA float32 contiguous tensors, a call wg_mr_check accepts, and
        WG_MR_ENGINE (read per call) not "0".  A synthesis call pays for this on the host before its first launch, so nothing here walks
        the module tree: the table and the module list come from the cached slots, and the parameters' dtype and device are looked at
        only when they are not the ones the engine has packed (`key`, what PackedWeights tracks: address and version of each)."""
        if os.environ.get("WG_MR_ENGINE") == "0":
            return "WG_MR_ENGINE=0", None, None
        if torch.is_grad_enabled():
            return "autograd is enabled", None, None
        table = self.mr_table()
        for m in self._mr_table.modules():
            if m.training:
                return "a module is in train()", None, None
        if x.dim() != 2 or h.dim() != 3 or x.size(0) != h.size(0) or h.size(1) != self.n_mels:
            return "not audio [B, N] with conditioning [B, n_mels, frames]", None, None
        eng = self.mr_engine()
        key = eng.packed.key_of(table)
        packed = key == eng.packed.key and eng.packed.buf is not None       # these very tensors were packed: float32, on buf's device
        if not packed and any(t is not None and t.dtype != torch.float32 for t in table):
            return "parameters are not float32", None, None
        rc = eng.check(x.size(0), x.size(1), h.size(2))
        if rc:
            return "wg_mr_check: code %d" % rc, None, None
        if not (x.is_cuda and x.dtype == torch.float32 and h.dtype == torch.float32 and h.device == x.device and
                (eng.packed.buf.device == x.device if packed else all(t is None or t.device == x.device for t in table))):
            return "tensors are not float32 on one HIP device", None, None
        if not (x.is_contiguous() and h.is_contiguous()):
            return "tensors are not contiguous", None, None
        return None, table, key

    def _engine_pass(self, x, h, inverse):
        """forward_computation / reverse_computation as one library call (wg_mr_forward / wg_mr_inverse), or None: the module path runs.
        The caller's tensors are only read."""
        why, table, key = self._engine_route(x, h)
        if why is not None:
            return None
        return self.mr_engine().run(table, x, h, inverse, key)        # (autograd is disabled: the parameters need no detach())

    def _check(self, x: Tensor, h: Tensor) -> int:
        """The number of columns T of x [B, N] as [B, n_group, T]; WgError for what the kernels would refuse, before any launch."""
        if x.dim() != 2 or h.dim() != 3 or h.size(0) != x.size(0) or h.size(1) != self.n_mels:
            raise WgError("MRWaveGlow expects audio [B, N] and conditioning [B, %d, frames], got %s and %s"
                          % (self.n_mels, tuple(x.shape), tuple(h.shape)))
        if x.size(1) < 1 or x.size(1) % self.n_group:
            raise WgError("MRWaveGlow: %d samples are no positive multiple of n_group %d" % (x.size(1), self.n_group))
        T = x.size(1) // self.n_group
        if T > h.size(2) * self.upsample_factor:          # assert x.size(2) <= y.size(2)  (mr_waveglow.py:65, :99)
            raise WgError("MRWaveGlow: %d frames upsample to %d columns, the audio has %d" % (h.size(2), h.size(2) * self.upsample_factor, T))
        engine.require_device(x, h)
        return T

    def forward_computation(self, x: Tensor, h: Tensor) -> Tuple[Tensor, Tensor]:
        out = self._engine_pass(x, h, False)
        if out is not None:
            return out
        T = self._check(x, h)
        B, s = x.size(0), self.upsample_factor
        if self.levels == 1:
            x, = _Unpack.apply(x, self.n_group, (self.n_group,))
        else:
            x = x.view(B, -1, self.n_group).transpose(1, 2)           # read through its strides by the first split: never copied, never freed
        emitted = []
        logdet = 0
        for level in range(self.levels - 1):
            x_diff, x, cond = _LevelSplit.apply(x, None if self.super_resolution else h, s, level == 0)
            for invconv, coupling in zip(self.invconv1x1_list[level], self.WNs_list[level]):
                x_diff, log_det_W = invconv(x_diff)
                x_diff, log_s = coupling(x_diff, cond)
                logdet = logdet + log_det_W + log_s.sum((1, 2))
            emitted.append(x_diff)
        if self.prior_flows:
            y = _Upsample.apply(h, None, s, T)
        for invconv, coupling in zip(self.prior_invconv1x1, self.prior_WNs):
            x, log_det_W = invconv(x)
            x, log_s = coupling(x, y)
            logdet = logdet + log_det_W + log_s.sum((1, 2))
        emitted.append(x)
        return _Pack.apply(self.n_group, *emitted), logdet

    def reverse_computation(self, z: Tensor, h: Tensor) -> Tuple[Tensor, Tensor]:
        out = self._engine_pass(z, h, True)
        if out is not None:
            return out
        T = self._check(z, h)
        s = self.upsample_factor
        *remained, z = _Unpack.apply(z, self.n_group, tuple(self.z_split_sizes))
        logdet = 0
        if self.prior_flows:
            y = _Upsample.apply(h, None, s, T)
        for invconv, coupling in zip(self.prior_invconv1x1[::-1], self.prior_WNs[::-1]):
            z, log_s = coupling.reverse(z, y)
            z, log_det_W = invconv.reverse(z)
            logdet = logdet + log_det_W + log_s.sum((1, 2))
        for level in range(self.levels - 2, -1, -1):
            z_diff = remained.pop()
            cond = z if self.super_resolution else _Upsample.apply(h, z, s, T)
            for invconv, coupling in zip(self.invconv1x1_list[level][::-1], self.WNs_list[level][::-1]):
                z_diff, log_s = coupling.reverse(z_diff, cond)
                z_diff, log_det_W = invconv.reverse(z_diff)
                logdet = logdet + log_det_W + log_s.sum((1, 2))
            z = _Merge.apply(z, z_diff, level == 0)
        if self.levels == 1:
            return _Pack.apply(self.n_group, z), logdet
        return z.transpose(1, 2).reshape(z.size(0), -1), logdet      # (the last merge wrote the audio's layout: a view, no copy)
