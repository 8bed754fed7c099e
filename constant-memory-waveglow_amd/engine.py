"""Thin torch-side plumbing over the C ABI: device buffers, streams, caches.  No arithmetic happens here.

Everything that computes is a HIP kernel behind include/wgflow.h.  PyTorch only owns the device memory
(tensors as workspaces / packed-weight buffers) and the stream the kernels are enqueued on.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import WgConfig, WgWnDims, WgError, check


_CAPTURE_LOCK = __import__("threading").Lock()


def _graph_mode():
    """How synthesis calls use hipGraphs (WG_GRAPHS): "0" never, "1" always (captured on the first call of a shape), unset = auto: a small
    call (at most 65 536 samples: ~250 launches of a few microseconds each) whose exact shape and buffers have been seen twice before is
    captured on its third occurrence and replayed from then on.  Measured on MI355X (gpurun_out/r04f_stdout.txt): one 0.7 s utterance
    between two synchronisations 2.72 -> 2.62 ms, host enqueue time 0.97 -> 0.26 ms; back to back the device is the bound either way
    (2.47 / 2.44 ms).  Variable-length serving never repeats a shape three times in a row of cache entries and stays on direct launches."""
    import os
    v = os.environ.get("WG_GRAPHS", "auto")
    return v if v in ("0", "1") else "auto"


def _stream(device=None):
    """the stream the kernels are enqueued on: torch's current stream OF THE TENSORS' DEVICE (not of the current device)"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device(fn):
    """Runs an engine entry point with the device of its first tensor argument current: the library sizes its launches with
    hipGetDevice and torch's allocations / streams follow the current device, so a model on cuda:1 must not be driven from
    cuda:0's context."""
    import functools

    def first_tensor(xs):
        for a in xs:
            if torch.is_tensor(a):
                return a
            if isinstance(a, (list, tuple)):
                t = first_tensor(a)
                if t is not None:
                    return t
        return None

    @functools.wraps(fn)
    def run(*args, **kwargs):
        t = first_tensor(args) if args else None
        if t is None:
            t = first_tensor(list(kwargs.values()))
        if t is None or not t.is_cuda:
            return fn(*args, **kwargs)                  # require_device raises the proper error
        with torch.cuda.device(t.device):
            return fn(*args, **kwargs)
    return run


def require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise WgError("constant-memory-waveglow_amd runs on an MI355X (HIP) device only: got a %s tensor. "
                          "There is no CPU fallback." % t.device)
        if t.dtype != torch.float32:
            raise WgError("the HIP engine computes in float32 (got %s)" % t.dtype)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise WgError("tensors of one call sit on different devices (%s and %s)" % (dev, t.device))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _table(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else None
    return arr


def make_config(flows, n_group, n_early_every, n_early_size, hop_size, n_mels,
                residual_channels, dilation_channels, skip_channels, depth, radix, precision=None, reverse_mode=False, bias=False):
    up = hop_size // n_group                  # reference model/waveglow.py:125
    k = up * 2 + 1                            # :126
    pad = k // 2 - up // 2                    # :128-129
    return WgConfig(flows, n_group, n_early_every, n_early_size, n_mels, up, k, pad,
                    residual_channels, dilation_channels, skip_channels, depth, radix,
                    _lib.default_precision() if precision is None else precision, int(bool(reverse_mode)), 0, int(bool(bias)))


class _Buffers:
    """Zero-initialised device workspaces keyed by (device, tag, shape...).  The kernels keep the zero halo of
    every activation plane intact, so a workspace is zeroed once when it is allocated.  At most `keep` shapes stay
    resident (least recently used goes first), so variable-length inference does not pile up multi-GB buffers."""

    def __init__(self, keep=4):
        self._ws = {}
        self._keep = keep

    def get(self, key, nbytes, device):
        buf = self._ws.pop(key, None)
        if buf is None or buf.numel() < nbytes or buf.device != device:
            if nbytes == 0:
                raise WgError("configuration/shape rejected by the HIP engine (workspace query returned 0)")
            while len(self._ws) >= self._keep:
                self._ws.pop(next(iter(self._ws)))
            buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self._ws[key] = buf                      # (re)insert as most recently used
        return buf

    def clear(self):
        self._ws.clear()


class PackedWeights:
    """Materialised (weight-normed, k-major) weights; re-packed only when a parameter changed."""

    def __init__(self):
        self.buf = None
        self.key = None
        self._pending = None

    @staticmethod
    def key_of(params):
        return tuple((p.data_ptr(), p._version) if p is not None else None for p in params)

    def stale(self, params, key=None):
        """True: `params` differ from what `buf` holds.  The buffer then counts as EMPTY until commit(): a pack that raises half way
        (a CPU or half parameter further down the table, an unsupported configuration, a failed launch) must not leave a key behind
        under which a retry would run on the old or half-written weights.  `key`: key_of(params), where the caller has it already."""
        if key is None:
            key = self.key_of(params)
        if key != self.key or self.buf is None:
            self.key, self._pending = None, key
            return True
        return False

    def commit(self):
        """the pack behind the last stale() succeeded"""
        self.key = self._pending


class _InverseGraphs:
    """The WG_GRAPHS / auto-capture policy of a model's synthesis call, shared by the engines that have one (ModelEngine, MelGlowEngine,
    MRWaveGlowEngine).
    `launch(z, h) -> (out, logdet)` enqueues the whole call on the current stream and allocates its two outputs."""

    def __init__(self):
        self._graphs = {}                        # (device, shape, frames, packed buffer, workspace) -> captured inverse (hipGraph)
        self._graph_seen = {}                    # auto mode: how often a small call's key has occurred

    def _run_inverse(self, key, launch, z, h):
        """Direct launches, or (see _graph_mode) the captured call replayed."""
        mode = _graph_mode()
        if mode != "0" and not torch.cuda.is_current_stream_capturing():
            if mode == "1" or key in self._graphs:
                return self._replay_inverse(key, launch, z, h)
            if z.numel() <= 65536:                          # auto: capture a small call on its third occurrence
                n = self._graph_seen.get(key, 0) + 1
                if len(self._graph_seen) > 16:
                    self._graph_seen.clear()
                self._graph_seen[key] = n
                if n >= 3:
                    try:
                        return self._replay_inverse(key, launch, z, h)
                    except Exception:                       # noqa: BLE001 -- a capture that fails only costs the graph: direct launches go on
                        self._graph_seen[key] = -(1 << 30)
        return launch(z, h)

    def _replay_inverse(self, key, launch, z, h):
        """The whole inverse call (~250 launches) captured once per shape into a hipGraph (torch.cuda.CUDAGraph on the stream the C ABI
        enqueues on) and replayed; the packed weights and the workspace are referenced by address, so a re-pack in place is seen."""
        ent = self._graphs.get(key)
        if ent is None:
            sz, sh = z.clone(), h.clone()
            launch(sz, sh)                                          # warm-up outside capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            # thread_local: only THIS thread's calls are illegal during the capture -- another thread of the process (a serving thread,
            # an nn.DataParallel replica sharing this engine) that allocates or launches meanwhile is left alone; one capture at a time
            with _CAPTURE_LOCK, torch.cuda.graph(graph, capture_error_mode="thread_local"):
                out, logdet = launch(sz, sh)
            while len(self._graphs) >= 4:
                self._graphs.pop(next(iter(self._graphs)))
            ent = self._graphs[key] = (graph, sz, sh, out, logdet)
        graph, sz, sh, out, logdet = ent
        sz.copy_(z)
        sh.copy_(h)
        graph.replay()
        return out.clone(), logdet.clone()


class ModelEngine(_InverseGraphs):
    """Whole-model entry points (wg_pack_weights / wg_forward / wg_inverse / wg_backward)."""

    def __init__(self, cfg: WgConfig):
        super().__init__()
        self.cfg = cfg
        self.cfg_keep = WgConfig.from_buffer_copy(cfg)      # the same model in stored-activation mode (memory_efficient=False)
        self.cfg_keep.keep_activations = 1
        self._kept_gen = 0                                  # bumped by every call that rewrites a stored-activation workspace
        self.buffers = _Buffers()
        self.packed = PackedWeights()
        self.n_params = None

    def _pack(self, params, device):
        L = _lib.lib()
        if self.n_params is None:
            self.n_params = L.wg_param_count(C.byref(self.cfg))
        if len(params) != self.n_params:
            raise WgError("parameter table has %d entries, expected %d" % (len(params), self.n_params))
        if self.packed.stale(params) or self.packed.buf.device != device:
            require_device(*params)
            nbytes = L.wg_packed_bytes(C.byref(self.cfg))
            if nbytes == 0:
                raise WgError("WaveGlow configuration not supported by the HIP kernels "
                              "(channels must be multiples of 32, odd radix <= 9, n_group <= 32)")
            if self.packed.buf is None or self.packed.buf.numel() < nbytes or self.packed.buf.device != device:
                self.packed.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            check(L.wg_pack_weights(C.byref(self.cfg), _table(params), _p(self.packed.buf), _stream()), "wg_pack_weights")
            self.packed.commit()
        return self.packed.buf

    def _ws(self, B, N, mode, device):
        nbytes = _lib.lib().wg_workspace_bytes(C.byref(self.cfg), B, N, mode)
        return self.buffers.get((device, mode, B, N), nbytes, device)

    def _ws_keep(self, B, N, device):
        nbytes = _lib.lib().wg_workspace_bytes(C.byref(self.cfg_keep), B, N, 1)
        return self.buffers.get((device, "keep", B, N), nbytes, device)

    def _launch(self, pk, ws, x, h, inverse, cfg=None):
        B, N = x.shape
        out = torch.empty_like(x)
        logdet = torch.empty(B, dtype=torch.float32, device=x.device)
        fn = _lib.lib().wg_inverse if inverse else _lib.lib().wg_forward
        check(fn(C.byref(cfg or self.cfg), _p(pk), _p(x), _p(h), B, N, h.shape[2], _p(out), _p(logdet), _p(ws), ws.numel(), _stream()),
              "wg_inverse" if inverse else "wg_forward")
        return out, logdet

    @on_device
    def run_keep(self, params, x, h):
        """wg_forward in stored-activation mode.  Returns (z, logdet, kept): `kept` = (generation, workspace) names the
        activations this call left behind; `backward(kept=...)` uses them if no later call overwrote them."""
        require_device(x, h, *params)
        x, h = x.contiguous(), h.contiguous()
        B, N = x.shape
        pk = self._pack(params, x.device)
        ws = self._ws_keep(B, N, x.device)
        self._kept_gen += 1
        z, logdet = self._launch(pk, ws, x, h, False, self.cfg_keep)
        return z, logdet, (self._kept_gen, ws)

    @on_device
    def run(self, params, x, h, inverse):
        require_device(x, h, params[0])            # (the whole table is checked when it is packed: _pack)
        x, h = x.contiguous(), h.contiguous()
        B, N = x.shape
        pk = self._pack(params, x.device)
        ws = self._ws(B, N, 0, x.device)
        if inverse:
            key = (x.device, tuple(x.shape), h.shape[2], pk.data_ptr(), ws.data_ptr())
            return self._run_inverse(key, lambda sz, sh: self._launch(pk, ws, sz, sh, True), x, h)
        return self._launch(pk, ws, x, h, False)

    @on_device
    def backward(self, params, z, h, dz, dlogdet, need, need_dh, need_dx, want_x=False, grads_out=None, flow_events=None,
                 kept=None):
        """need[i]: produce the gradient of params[i] (into grads_out[i] when given).  Returns (grads, dh, dx, x_rebuilt).
        kept: what run_keep returned for this z; still-valid stored activations are used, overwritten ones fall back to
        the recomputing backward (same gradients, one extra WN forward per flow)."""
        require_device(z, h, dz, dlogdet)
        z, h, dz, dlogdet = z.contiguous(), h.contiguous(), dz.contiguous(), dlogdet.contiguous()
        B, N = z.shape
        F = h.shape[2]
        pk = self._pack(params, z.device)
        cfg = self.cfg
        if kept is not None and kept[0] == self._kept_gen:
            cfg, ws = self.cfg_keep, kept[1]
            self._kept_gen += 1                             # the backward rebuilds X in place: the stored state is spent
        else:
            ws = self._ws(B, N, 1, z.device)
        if grads_out is not None:
            grads = [g if nd else None for g, nd in zip(grads_out, need)]
        else:
            grads = [torch.empty_like(p) if (p is not None and nd) else None for p, nd in zip(params, need)]
        dh = torch.empty_like(h) if need_dh else None
        dx = torch.empty_like(z) if need_dx else None
        xr = torch.empty_like(z) if want_x else None
        check(_lib.lib().wg_backward(C.byref(cfg), _table(params), _p(pk), _p(z), _p(h), _p(dz), _p(dlogdet), B, N, F,
                                     _table(grads), _p(dh), _p(dx), _p(xr), _p(ws), ws.numel(), _stream(),
                                     self._events(flow_events)), "wg_backward")
        return grads, dh, dx, xr

    @on_device
    def train_step(self, params, x, h, sigma, elementwise_mean, need, grads_out=None, need_dh=False, flow_events=None,
                   keep=False, metrics=None):
        """wg_train_step: forward + NLL + backward in one call (the forward keeps the last flow's layers for the backward;
        keep=True -- memory_efficient=False -- keeps every flow's, so no WN is recomputed).
        metrics (optional, 4 device floats): receives the logged scalars [logdet/numel, z.mean, z.std, loss] (lightning.py:58-64).
        Returns (loss, z, logdet, grads, dh)."""
        require_device(x, h, *params)
        x, h = x.contiguous(), h.contiguous()
        B, N = x.shape
        pk = self._pack(params, x.device)
        cfg = self.cfg_keep if keep else self.cfg
        if keep:
            ws = self._ws_keep(B, N, x.device)
            self._kept_gen += 1
        else:
            ws = self._ws(B, N, 1, x.device)
        scratch = self.buffers.get((x.device, "step", B, N), 4 * _lib.lib().wg_train_scratch_floats(B, N), x.device)
        if grads_out is not None:
            grads = [g if nd else None for g, nd in zip(grads_out, need)]
        else:
            grads = [torch.empty_like(p) if (p is not None and nd) else None for p, nd in zip(params, need)]
        z = torch.empty_like(x)
        logdet = torch.empty(B, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dh = torch.empty_like(h) if need_dh else None
        check(_lib.lib().wg_train_step(C.byref(cfg), _table(params), _p(pk), _p(x), _p(h), B, N, h.shape[2], float(sigma),
                                       int(elementwise_mean), _p(z), _p(logdet), _p(loss), _p(metrics), _table(grads), _p(dh), _p(scratch),
                                       _p(ws), ws.numel(), _stream(), self._events(flow_events)), "wg_train_step")
        return loss, z, logdet, grads, dh

    @staticmethod
    def _events(events):
        """torch.cuda.Event list -> array of raw hipEvent_t (NULL when not given)"""
        if not events:
            return None
        arr = (C.c_void_p * len(events))()
        for i, e in enumerate(events):
            arr[i] = e.cuda_event
        return arr

    @on_device
    def upsample(self, params, h, T):
        require_device(h)
        h = h.contiguous()
        B, M, F = h.shape
        pk = self._pack(params, h.device)
        y = torch.empty(B, M, T, dtype=torch.float32, device=h.device)
        check(_lib.lib().wg_upsample(C.byref(self.cfg), _p(pk), _p(h), B, F, T, _p(y), _stream()), "wg_upsample")
        return y


class CouplingEngine:
    """Block-level entry points for AffineCouplingBlock(WN) / WN."""

    def __init__(self, dims: WgWnDims):
        self.dims = dims
        self.buffers = _Buffers()
        self.packed = PackedWeights()

    def _pack(self, params, device):
        L = _lib.lib()
        if self.packed.stale(params) or self.packed.buf.device != device:
            nbytes = L.wg_wn_packed_bytes(C.byref(self.dims))
            if nbytes == 0:
                raise WgError("WN configuration not supported by the HIP kernels "
                              "(channels must be multiples of 32, odd radix <= 9, in_channels <= 16)")
            if self.packed.buf is None or self.packed.buf.numel() < nbytes or self.packed.buf.device != device:
                self.packed.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            check(L.wg_wn_pack_weights(C.byref(self.dims), _table(params), _p(self.packed.buf), _stream()), "wg_wn_pack_weights")
            self.packed.commit()
        return self.packed.buf

    def _ws(self, B, T, mode, device):
        nbytes = _lib.lib().wg_coupling_workspace_bytes(C.byref(self.dims), B, T, mode)
        return self.buffers.get((device, mode, B, T), nbytes, device)

    @on_device
    def apply(self, params, x, y, reverse):
        require_device(x, y, *params)
        x, y = x.contiguous(), y.contiguous()
        B, c, T = x.shape
        if y.shape[2] != T or y.shape[1] != self.dims.aux_ch or c != 2 * self.dims.in_ch:
            raise WgError("coupling: x %s / y %s do not match the block's dimensions" % (tuple(x.shape), tuple(y.shape)))
        pk = self._pack(params, x.device)
        ws = self._ws(B, T, 0, x.device)
        z = torch.empty_like(x)
        log_s = torch.empty(B, c // 2, T, dtype=torch.float32, device=x.device)
        check(_lib.lib().wg_coupling_apply(C.byref(self.dims), _p(pk), _p(x), _p(y), B, T, int(reverse), _p(z), _p(log_s),
                                           _p(ws), ws.numel(), _stream()), "wg_coupling_apply")
        return z, log_s

    @on_device
    def wn(self, params, x, y):
        require_device(x, y, *params)
        x, y = x.contiguous(), y.contiguous()
        B, ic, T = x.shape
        pk = self._pack(params, x.device)
        ws = self._ws(B, T, 0, x.device)
        log_s, t = torch.empty_like(x), torch.empty_like(x)
        check(_lib.lib().wg_wn_apply(C.byref(self.dims), _p(pk), _p(x), _p(y), B, T, _p(log_s), _p(t), _p(ws), ws.numel(),
                                     _stream()), "wg_wn_apply")
        return log_s, t

    @on_device
    def backward(self, params, z, y, dz, dlog_s, reverse, need, need_dy, x_out):
        require_device(z, y, dz, dlog_s)
        z, y, dz, dlog_s = z.contiguous(), y.contiguous(), dz.contiguous(), dlog_s.contiguous()
        B, c, T = z.shape
        pk = self._pack(params, z.device)
        ws = self._ws(B, T, 1, z.device)
        grads = [torch.empty_like(p) if (p is not None and nd) else None for p, nd in zip(params, need)]
        dx = torch.empty_like(z)
        dy = torch.empty_like(y) if need_dy else None
        check(_lib.lib().wg_coupling_backward(C.byref(self.dims), _table(params), _p(pk), _p(z), _p(y), _p(dz), _p(dlog_s), B, T,
                                              int(reverse), _p(x_out), _p(dx), _p(dy), _table(grads), _p(ws), ws.numel(),
                                              _stream()), "wg_coupling_backward")
        return dx, dy, grads


_INV_BUFFERS = _Buffers()
_LAYER_BUFFERS = _Buffers()


@on_device
def layer_apply(dims, params, x, y):
    """NonCausalLayer.forward on its own (model/waveglow.py:41-46; wg_layer_apply): params = [W.g or None, W.v, W_o.g or None, W_o.v].
    Returns (res or None, skip)."""
    require_device(x, y, *params)
    x, y = x.contiguous(), y.contiguous()
    if dims.rows > 0:                                        # NonCausalLayer2D: x [B, C, H, W], y [B, 2 Cd, 1, W]
        B, Cin, H, T = x.shape
        if Cin != dims.res_ch or H != dims.rows or tuple(y.shape) != (B, 2 * dims.dil_ch, 1, T):
            raise WgError("NonCausalLayer2D: x %s / y %s do not match the layer (x [B, %d, H, W], y [B, %d, 1, W])"
                          % (tuple(x.shape), tuple(y.shape), dims.res_ch, 2 * dims.dil_ch))
    else:
        B, Cin, T = x.shape
        if Cin != dims.res_ch or tuple(y.shape) != (B, 2 * dims.dil_ch, T):
            raise WgError("NonCausalLayer: x %s / y %s do not match the layer (x [B, %d, T], y [B, %d, T])"
                          % (tuple(x.shape), tuple(y.shape), dims.res_ch, 2 * dims.dil_ch))
    nbytes = _lib.lib().wg_layer_workspace_bytes(C.byref(dims), B, T)
    if nbytes == 0:
        raise WgError("NonCausalLayer shape not supported by the HIP kernels (residual / skip channels multiples of 16, dilation channels "
                      "a multiple of 32, odd radix <= 9)")
    ws = _LAYER_BUFFERS.get((x.device, dims.res_ch, dims.dil_ch, dims.skip_ch, dims.radix, dims.dilation, dims.h_dilation, dims.rows, B, T), nbytes, x.device)
    res = None if dims.last_layer else torch.empty_like(x)
    skip = torch.empty((B, dims.skip_ch) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    check(_lib.lib().wg_layer_apply(C.byref(dims), _table([None if p is None else p.contiguous() for p in params]), _p(x), _p(y), B, T, _p(res),
                                    _p(skip), _p(ws), ws.numel(), _stream()), "wg_layer_apply")
    return res, skip


@on_device
def affine_apply(xb, log_s, t, reverse):
    """The coupling's own arithmetic on plain tensors (wg_affine_apply): xb * exp(log_s) + t, or (reverse) (xb - t) / exp(log_s)."""
    require_device(xb, log_s, t)
    xb, log_s, t = xb.contiguous(), log_s.contiguous(), t.contiguous()
    if not (xb.shape == log_s.shape == t.shape) or xb.dtype != torch.float32 or log_s.dtype != torch.float32 or t.dtype != torch.float32:
        raise WgError("affine coupling: the transform must return float32 (log_s, t) of the shape of the passed half, got %s / %s for %s"
                      % (tuple(log_s.shape), tuple(t.shape), tuple(xb.shape)))
    out = torch.empty_like(xb)
    check(_lib.lib().wg_affine_apply(_p(xb), _p(log_s), _p(t), xb.numel(), int(reverse), _p(out), _stream()), "wg_affine_apply")
    return out


@on_device
def affine_backward(out_half, log_s, t, dout, dlog_s, reverse):
    """wg_affine_backward -> (input half rebuilt, d/d log_s, d/d t of the transform's outputs, gradient of the input half)."""
    require_device(out_half, log_s, t, dout)
    out_half, log_s, t, dout = out_half.contiguous(), log_s.contiguous(), t.contiguous(), dout.contiguous()
    dlog_s = None if dlog_s is None else dlog_s.contiguous()
    rebuilt, g_ls, g_t, din = (torch.empty_like(out_half) for _ in range(4))
    check(_lib.lib().wg_affine_backward(_p(out_half), _p(log_s), _p(t), _p(dout), _p(dlog_s), out_half.numel(), int(reverse), _p(rebuilt),
                                        _p(g_ls), _p(g_t), _p(din), _stream()), "wg_affine_backward")
    return rebuilt, g_ls, g_t, din


@on_device
def layer_backward(dims, params, x, y, dres, dskip, need, need_dx, need_dy):
    """wg_layer_backward: (dx, dy, [dW.g, dW.v, dW_o.g, dW_o.v]) of NonCausalLayer / NonCausalLayer2D called on its own; None where not needed."""
    require_device(x, y, dskip, *params)
    x, y, dskip = x.contiguous(), y.contiguous(), dskip.contiguous()
    dres = None if dres is None else dres.contiguous()
    B, T = x.shape[0], x.shape[-1]
    nbytes = _lib.lib().wg_layer_backward_workspace_bytes(C.byref(dims), B, T)
    if nbytes == 0:
        raise WgError("NonCausalLayer shape not supported by the HIP kernels")
    ws = _LAYER_BUFFERS.get((x.device, "bwd", dims.res_ch, dims.dil_ch, dims.skip_ch, dims.radix, dims.dilation, dims.h_dilation, dims.rows, B, T), nbytes, x.device)
    params = [None if p is None else p.contiguous() for p in params]
    grads = [torch.empty_like(p) if (p is not None and nd) else None for p, nd in zip(params, need)]
    dx = torch.empty_like(x) if need_dx else None
    dy = torch.empty_like(y) if need_dy else None
    check(_lib.lib().wg_layer_backward(C.byref(dims), _table(params), _p(x), _p(y), _p(dres), _p(dskip), B, T, _p(dx), _p(dy), _table(grads),
                                       _p(ws), ws.numel(), _stream()), "wg_layer_backward")
    return dx, dy, grads


class LayerFn(torch.autograd.Function):
    """NonCausalLayer / NonCausalLayer2D forward on its own as an autograd node: wg_layer_apply / wg_layer_backward."""

    @staticmethod
    def forward(ctx, x, y, dims, *params):
        res, skip = layer_apply(dims, [None if p is None else p.detach() for p in params], x.detach(), y.detach())
        ctx.dims, ctx.n = dims, len(params)
        ctx.save_for_backward(x, y, *[p for p in params if p is not None])
        ctx.present = [p is not None for p in params]
        return (skip,) if res is None else (res, skip)

    @staticmethod
    def backward(ctx, *douts):
        x, y = ctx.saved_tensors[:2]
        it = iter(ctx.saved_tensors[2:])
        params = [next(it) if here else None for here in ctx.present]
        dres, dskip = (None, douts[0]) if len(douts) == 1 else douts
        need = [p is not None and ctx.needs_input_grad[3 + k] for k, p in enumerate(params)]
        dx, dy, grads = layer_backward(ctx.dims, [None if p is None else p.detach() for p in params], x.detach(), y.detach(), dres, dskip, need,
                                       ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (dx, dy, None) + tuple(grads)


@on_device
def invconv_apply(W, x, reverse):
    require_device(W, x)
    x = x.contiguous()
    B, c, T = x.shape
    Wm = W.reshape(c, c).contiguous()
    nbytes = _lib.lib().wg_invconv_workspace_bytes(c, B, T)
    ws = _INV_BUFFERS.get((x.device, c, B, T), nbytes, x.device)
    z = torch.empty_like(x)
    logdet = torch.empty((), dtype=torch.float32, device=x.device)
    check(_lib.lib().wg_invconv_apply(_p(Wm), c, _p(x), B, T, int(reverse), _p(z), _p(logdet), _p(ws), ws.numel(), _stream()),
          "wg_invconv_apply")
    return z, logdet


@on_device
def invconv_backward(W, z, dz, dlogdet, reverse, x_out):
    require_device(W, z, dz, dlogdet)
    z, dz = z.contiguous(), dz.contiguous()
    B, c, T = z.shape
    Wm = W.reshape(c, c).contiguous()
    nbytes = _lib.lib().wg_invconv_workspace_bytes(c, B, T)
    ws = _INV_BUFFERS.get((z.device, c, B, T), nbytes, z.device)
    dx = torch.empty_like(z)
    dW = torch.empty(c, c, dtype=torch.float32, device=z.device)
    check(_lib.lib().wg_invconv_backward(_p(Wm), c, _p(z), _p(dz), _p(dlogdet.contiguous()), B, T, int(reverse), _p(x_out), _p(dx),
                                         _p(dW), _p(ws), ws.numel(), _stream()), "wg_invconv_backward")
    return dx, dW


@on_device
def nll_loss(z, logdet, sigma, elementwise_mean, metrics=None):
    """loss (device scalar); metrics (optional, 4 device floats) receives [logdet.sum()/z.numel(), z.mean(), z.std(), loss]."""
    require_device(z, logdet, metrics)
    z, logdet = z.contiguous(), logdet.contiguous()
    B, N = z.shape
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    scratch = torch.empty(_lib.lib().wg_nll_scratch_floats(B), dtype=torch.float32, device=z.device)
    check(_lib.lib().wg_nll_loss(_p(z), _p(logdet), B, N, float(sigma), int(elementwise_mean), _p(loss), _p(metrics), _p(scratch),
                                 _stream()), "wg_nll_loss")
    return loss


def training_metrics(z, logdet, sigma=1.0, elementwise_mean=True):
    """The scalars LightModel.training_step logs (model/lightning.py:58-64) as ONE device vector
    [logdet.sum() / z.numel(), z.mean(), z.std(), loss]; a data-parallel caller mean-reduces it (sync_dist=True)."""
    m = torch.empty(4, dtype=torch.float32, device=z.device)
    nll_loss(z, logdet, sigma, elementwise_mean, metrics=m)
    return m


@on_device
def nll_loss_backward(z, sigma, elementwise_mean, dloss):
    require_device(z, dloss)
    z = z.contiguous()
    B, N = z.shape
    dz = torch.empty_like(z)
    dlogdet = torch.empty(B, dtype=torch.float32, device=z.device)
    check(_lib.lib().wg_nll_loss_backward(_p(z), B, N, float(sigma), int(elementwise_mean), _p(dloss.contiguous()), _p(dz),
                                          _p(dlogdet), _stream()), "wg_nll_loss_backward")
    return dz, dlogdet


# ---- WSRGlow conditioning front-end (include/wgflow.h: wg_wsr_cond*) -----------------------------------------------------
WSR_COND_CHANNELS = 8 * 400 + 9 * 51


@on_device
def wsr_cond(c, mu_table, ang_table):
    """c[B,L] -> cond[B,3659,L/8]  (WSRGlow._get_cond, model/wsrglow.py:37-50; c is read clipped, not modified)."""
    require_device(c, mu_table, ang_table)
    if c.dim() != 2 or c.size(1) % 8 or c.size(1) < 8:
        raise WgError("WSRGlow conditioning signal must be [B, L] with L a multiple of 8")
    if tuple(mu_table.shape) != (256, 400) or tuple(ang_table.shape) != (120, 50):
        raise WgError("WSRGlow embedding tables must be [256,400] and [120,50]")
    c, mu_table, ang_table = c.contiguous(), mu_table.contiguous(), ang_table.contiguous()
    B, L = c.shape
    cond = torch.empty(B, WSR_COND_CHANNELS, L // 8, dtype=torch.float32, device=c.device)
    check(_lib.lib().wg_wsr_cond(_p(c), B, L, _p(mu_table), _p(ang_table), _p(cond), _stream()), "wg_wsr_cond")
    return cond


@on_device
def wsr_cond_pre(c):
    """Diagnostics (wg_wsr_cond_pre): the quantisers' float32 values before truncation -> (mu_pre[B,L], ang_pre[B,9,L/8])."""
    require_device(c)
    c = c.contiguous()
    B, L = c.shape
    mu_pre = torch.empty(B, L, dtype=torch.float32, device=c.device)
    ang_pre = torch.empty(B, 9, L // 8, dtype=torch.float32, device=c.device)
    check(_lib.lib().wg_wsr_cond_pre(_p(c), B, L, _p(mu_pre), _p(ang_pre), _stream()), "wg_wsr_cond_pre")
    return mu_pre, ang_pre


@on_device
def wsr_cond_backward(c, dcond, out=None):
    """-> (d mu_table [256,400], d ang_table [120,50]) from dcond[B,3659,L/8]; out: optional pair of contiguous tensors to fill."""
    require_device(c, dcond)
    c, dcond = c.contiguous(), dcond.contiguous()
    B, L = c.shape
    if tuple(dcond.shape) != (B, WSR_COND_CHANNELS, L // 8):
        raise WgError("dcond must be [B, 3659, L/8]")
    if out is not None:
        dmu, dang = out
        require_device(dmu, dang)
        if tuple(dmu.shape) != (256, 400) or tuple(dang.shape) != (120, 50) or not (dmu.is_contiguous() and dang.is_contiguous()):
            raise WgError("wsr_cond_backward: out must be contiguous [256,400] and [120,50] tensors")
    else:
        dmu = torch.empty(256, 400, dtype=torch.float32, device=c.device)
        dang = torch.empty(120, 50, dtype=torch.float32, device=c.device)
    check(_lib.lib().wg_wsr_cond_backward(_p(c), B, L, _p(dcond), _p(dmu), _p(dang), _stream()), "wg_wsr_cond_backward")
    return dmu, dang


# ---- WaveFlow (include/wgflow.h: wg_wf_*) ------------------------------------------------------------------------------------
class WaveFlowEngine:
    """Whole-model entry points of WaveFlow: wg_wf_pack_weights / wg_wf_forward / wg_wf_inverse / wg_wf_backward."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.buffers = _Buffers()
        self.packed = PackedWeights()
        self._tape = None

    def _pack(self, params, device):
        L = _lib.lib()
        if len(params) != L.wg_wf_param_count(C.byref(self.cfg)):
            raise WgError("WaveFlow parameter table has %d entries" % len(params))
        if self.packed.stale(params) or self.packed.buf.device != device:
            require_device(*params)
            nbytes = L.wg_wf_packed_bytes(C.byref(self.cfg))
            if nbytes == 0:
                raise WgError("WaveFlow configuration not supported by the HIP kernels (n_group in {8,16,32,64,128}, channels "
                              "multiples of 32)")
            if self.packed.buf is None or self.packed.buf.numel() < nbytes or self.packed.buf.device != device:
                self.packed.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            check(L.wg_wf_pack_weights(C.byref(self.cfg), _table(params), _p(self.packed.buf), _stream()), "wg_wf_pack_weights")
            self.packed.commit()
        return self.packed.buf

    def _ws(self, B, N, mode, device):
        nbytes = _lib.lib().wg_wf_workspace_bytes(C.byref(self.cfg), B, N, mode)
        return self.buffers.get((device, mode, B, N), nbytes, device)

    @on_device
    def forward(self, params, x, mel, keep_tape):
        require_device(x, mel, *params)
        x, mel = x.contiguous(), mel.contiguous()
        B, N = x.shape
        pk = self._pack(params, x.device)
        ws = self._ws(B, N, 0, x.device)
        tape = None
        if keep_tape:
            # one tape PER forward call, owned by that call's autograd node: a second forward of the same shape before the first
            # backward (two losses, gradient accumulation, a grad-enabled evaluation pass) must not overwrite the flow inputs the
            # first backward recomputes from.  (zero-filled: the kernels keep the halo of every plane zero, they do not write it)
            nbytes = _lib.lib().wg_wf_tape_bytes(C.byref(self.cfg), B, N)
            tape = torch.zeros(nbytes, dtype=torch.uint8, device=x.device)
        z = torch.empty_like(x)
        logdet = torch.empty(B, dtype=torch.float32, device=x.device)
        check(_lib.lib().wg_wf_forward(C.byref(self.cfg), _table(params), _p(pk), _p(x), _p(mel), B, N, mel.shape[2], _p(z), _p(logdet),
                                       _p(tape), _p(ws), ws.numel(), _stream()), "wg_wf_forward")
        return z, logdet, tape

    @on_device
    def upsample(self, params, mel):
        """WaveFlow._upsample_h: mel [B, n_mels, F] -> [B, n_mels, F s - 2 (s // 2) + 2 s + 1]"""
        require_device(mel, *params)
        mel = mel.contiguous()
        B, M, F = mel.shape
        s = 256 // self.cfg.n_group
        T = F * s - 2 * (s // 2) + 2 * s + 1
        pk = self._pack(params, mel.device)
        y = torch.empty(B, M, T, dtype=torch.float32, device=mel.device)
        check(_lib.lib().wg_wf_upsample(C.byref(self.cfg), _table(params), _p(pk), _p(mel), B, F, T, _p(y), _stream()), "wg_wf_upsample")
        return y

    @on_device
    def inverse(self, params, z, mel):
        require_device(z, mel, *params)
        z, mel = z.contiguous(), mel.contiguous()
        B, N = z.shape
        pk = self._pack(params, z.device)
        ws = self._ws(B, N, 1, z.device)
        x = torch.empty_like(z)
        logdet = torch.empty(B, dtype=torch.float32, device=z.device)
        check(_lib.lib().wg_wf_inverse(C.byref(self.cfg), _table(params), _p(pk), _p(z), _p(mel), B, N, mel.shape[2], _p(x), _p(logdet),
                                       _p(ws), ws.numel(), _stream()), "wg_wf_inverse")
        return x, logdet

    @on_device
    def backward(self, params, tape, mel, dz, dlogdet, need_dmel, need_dx):
        require_device(mel, dz, dlogdet)
        mel, dz, dlogdet = mel.contiguous(), dz.contiguous(), dlogdet.contiguous()
        B, N = dz.shape
        pk = self._pack(params, dz.device)
        ws = self._ws(B, N, 1, dz.device)
        grads = [None if p is None else torch.empty_like(p) for p in params]
        dmel = torch.empty_like(mel) if need_dmel else None
        dx = torch.empty_like(dz) if need_dx else None
        check(_lib.lib().wg_wf_backward(C.byref(self.cfg), _table(params), _p(pk), _p(tape), _p(mel), _p(dz), _p(dlogdet), B, N,
                                        mel.shape[2], _table(grads), _p(dmel), _p(dx), _p(ws), ws.numel(), _stream()), "wg_wf_backward")
        return grads, dmel, dx


class WN2DEngine(WaveFlowEngine):
    """WN2D.forward on its own (wg_wf_wn_apply): the packing and workspaces of a one-flow WaveFlow whose upsampler entries are placeholders."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self._dummy = None

    def table(self, wn_params, device):
        if self._dummy is None or self._dummy[0].device != device:
            M, s = self.cfg.n_mels, 256 // self.cfg.n_group
            self._dummy = [torch.zeros(M, device=device), torch.ones(M, M, 2 * s + 1, device=device)]
        return [self._dummy[0], None, self._dummy[1]] + list(wn_params)

    @on_device
    def apply(self, wn_params, x, y):
        require_device(x, y, *wn_params)
        B, one, rows, W = x.shape
        if one != 1 or rows > self.cfg.n_group or tuple(y.shape) != (B, self.cfg.n_mels, W):
            raise WgError("WN2D: x %s / y %s do not match (x [B, 1, rows <= %d, W], y [B, %d, W])"
                          % (tuple(x.shape), tuple(y.shape), self.cfg.n_group, self.cfg.n_mels))
        x, y = x.contiguous(), y.contiguous()
        params = self.table(wn_params, x.device)
        pk = self._pack(params, x.device)
        ws = self._ws(B, W * self.cfg.n_group, 0, x.device)
        log_s, t = torch.empty_like(x), torch.empty_like(x)
        check(_lib.lib().wg_wf_wn_apply(C.byref(self.cfg), _table(params), _p(pk), _p(x), _p(y), B, rows, W, _p(log_s), _p(t), _p(ws),
                                        ws.numel(), _stream()), "wg_wf_wn_apply")
        return log_s, t

    @on_device
    def backward(self, wn_params, x, y, dlog_s, dt, need, need_dx, need_dy):
        """wg_wf_wn_backward: gradients of x / y (None where not needed) and of the WN2D parameters (`need`: per table entry)."""
        require_device(x, y, dlog_s, dt, *wn_params)
        x, y, dlog_s, dt = x.contiguous(), y.contiguous(), dlog_s.contiguous(), dt.contiguous()
        B, one, rows, W = x.shape
        params = self.table(wn_params, x.device)
        pk = self._pack(params, x.device)
        ws = self._ws(B, W * self.cfg.n_group, 1, x.device)
        grads = [None, None, None] + [torch.empty_like(p) if (p is not None and nd) else None for p, nd in zip(wn_params, need)]
        dx = torch.empty_like(x) if need_dx else None
        dy = torch.empty_like(y) if need_dy else None
        check(_lib.lib().wg_wf_wn_backward(C.byref(self.cfg), _table(params), _p(pk), _p(x), _p(y), _p(dlog_s), _p(dt), B, rows, W, _p(dx), _p(dy),
                                           _table(grads), _p(ws), ws.numel(), _stream()), "wg_wf_wn_backward")
        return dx, dy, grads[3:]


# ---- log-mel conditioner (include/wgflow.h: wg_melspec) -------------------------------------------------------------------------
@on_device
def melspec(x, sr, n_fft, hop, f_min, f_max, n_mels, return_power=False):
    """audio [B, N] -> log-mel [B, n_mels, N // hop + 1]  (MelSpec.forward, model/condition.py:18-19).
    return_power: also the power spectrogram [B, n_fft // 2 + 1, frames] the mel filters are applied to."""
    require_device(x)
    if x.dim() != 2:
        raise WgError("MelSpec expects audio [B, N]")
    x = x.contiguous()
    B, N = x.shape
    frames = _lib.lib().wg_melspec_frames(N, n_fft, hop)
    out = torch.empty(B, n_mels, frames, dtype=torch.float32, device=x.device)
    power = torch.empty(B, n_fft // 2 + 1, frames, dtype=torch.float32, device=x.device) if return_power else None
    check(_lib.lib().wg_melspec(_p(x), B, N, int(sr), int(n_fft), int(hop), float(f_min), float(f_max if f_max is not None else 0.0),
                                int(n_mels), _p(out), _p(power), _stream()), "wg_melspec")
    return (out, power) if return_power else out


@on_device
def lowpass(x, n_fft, hop, cut_bins, step):
    """x [B, T] -> STFT low-pass (bins >= cut_bins zeroed), every step-th sample: [B, ceil(T / step)]  (condition.py:22-66)."""
    require_device(x)
    if x.dim() != 2:
        raise WgError("LowPass expects audio [B, T]")
    x = x.contiguous()
    B, T = x.shape
    nbytes = _lib.lib().wg_lowpass_workspace_bytes(B, T, int(n_fft), int(hop))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=x.device)
    out = torch.empty(B, (T + step - 1) // step, dtype=torch.float32, device=x.device)
    check(_lib.lib().wg_lowpass(_p(x), B, T, int(n_fft), int(hop), int(cut_bins), int(step), _p(out), _p(ws), ws.numel(), _stream()), "wg_lowpass")
    return out


# ---- MelGlow building blocks (include/wgflow.h wg_mg_* / wg_lvc_*; kernels in csrc/wg_lvc.h) ----------------------------------------
def mg_gemm(A, B, out, M, N, K, a, b, c, batch=1, N1=None, K1=None, add=None, alpha=1.0, beta=1.0):
    """out[bt] = alpha A[bt] B[bt] (+ beta add[bt]) with the element strides a = (a_m, a_k, a_k2, a_b), b = (b_k, b_k2, b_n, b_n2, b_b),
    c = (c_m, c_n, c_n2, c_b) of wg_mg_gemm_desc; the tensors' data pointers are the origins.  A split-K product gets its partial-sum
    workspace from torch's caching allocator (wg_mg_gemm_workspace_bytes)."""
    d = _lib.WgMgGemmDesc(M, N, K, batch, N1 or N, K1 or K, *a, *b, *c, alpha, beta)
    L = _lib.lib()
    nbytes = L.wg_mg_gemm_workspace_bytes(C.byref(d))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=out.device) if nbytes else None
    check(L.wg_mg_gemm(C.byref(d), _p(A), _p(B), _p(add), _p(out), _p(ws), nbytes, _stream(out.device)), "wg_mg_gemm")
    return out


def mg_conv1x1(w, x, out=None, add=None, transpose=False):
    """1x1 conv batched over items: out[b] = w x[b] (+ add[b]); w [M, K] row-major (transpose: w is [K, M] and w^T is applied).
    x [B, K, T] contiguous."""
    Bn, K, T = x.shape
    M = w.size(1) if transpose else w.size(0)
    if out is None:
        out = torch.empty((Bn, M, T), dtype=torch.float32, device=x.device)
    a = (1, M, 0, 0) if transpose else (K, 1, 0, 0)
    return mg_gemm(w, x, out, M, T, K, a, (T, 0, 1, 0, K * T), (T, 1, 0, M * T), batch=Bn, add=add)


def mg_conv1x1_wgrad(dy, x, out):
    """out[M, K] = sum over items and positions of dy[b] x[b]^T (dy [B, M, T], x [B, K, T] contiguous; out rows contiguous)."""
    Bn, M, T = dy.shape
    K = x.size(1)
    return mg_gemm(dy, x, out, M, K, T * Bn, (T, 1, M * T, 0), (1, K * T, T, 0, 0), (K, 1, 0, 0), K1=T)


def mg_grouped(w, x, G, out=None, add=None, transpose=False):
    """Grouped 1x1 conv on [channels, N] activations: w [G * Mg, Kg] (transpose: the product with each group's w^T)."""
    Mg, Kg = w.size(0) // G, w.size(1)
    Mo, Ko = (Kg, Mg) if transpose else (Mg, Kg)
    N = x.size(1)
    if out is None:
        out = torch.empty((G * Mo, N), dtype=torch.float32, device=x.device)
    a = (1, Kg, 0, Mg * Kg) if transpose else (Kg, 1, 0, Mg * Kg)
    return mg_gemm(w, x, out, Mo, N, Ko, a, (N, 0, 1, 0, Ko * N), (N, 1, 0, Mo * N), batch=G, add=add)


def mg_grouped_wgrad(dy, x, G, out):
    """out[G * Mg, Kg] = per group dy_g x_g^T over the N columns (dy [G * Mg, N], x [G * Kg, N])."""
    N = dy.size(1)
    Mg, Kg = dy.size(0) // G, x.size(0) // G
    return mg_gemm(dy, x, out, Mg, Kg, N, (N, 1, 0, Mg * N), (1, 0, N, 0, Kg * N), (Kg, 1, 0, Mg * Kg), batch=G)


def mg_bn_stats(x, eps, train, running_mean, running_var):
    Cn, N = x.shape
    mean, invstd = (torch.empty(Cn, dtype=torch.float64, device=x.device) for _ in range(2))     # double: wgflow.h wg_mg_bn_stats
    var_unb = torch.empty(Cn, dtype=torch.float32, device=x.device)
    check(_lib.lib().wg_mg_bn_stats(_p(x), Cn, N, float(eps), int(train), _p(running_mean), _p(running_var), _p(mean), _p(invstd),
                                    _p(var_unb), _stream(x.device)), "wg_mg_bn_stats")
    return mean, invstd, var_unb


def mg_bn_update(running_mean, running_var, num_batches_tracked, mean, var_unb, momentum):
    check(_lib.lib().wg_mg_bn_update(_p(running_mean), _p(running_var), _p(num_batches_tracked), _p(mean), _p(var_unb), mean.numel(),
                                     float(momentum), _stream(mean.device)), "wg_mg_bn_update")


def mg_bn_tanh(x, mean, invstd, gamma, beta, res=None):
    Cn, N = x.shape
    s = torch.empty_like(x)
    total = torch.empty_like(x) if res is not None else None
    check(_lib.lib().wg_mg_bn_tanh(_p(x), Cn, N, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(res), _p(s), _p(total),
                                   _stream(x.device)), "wg_mg_bn_tanh")
    return s, total


def mg_bn_tanh_backward(ds, s, x, mean, invstd, gamma, train, dgamma=None, dbeta=None):
    Cn, N = x.shape
    dx = torch.empty_like(x)
    check(_lib.lib().wg_mg_bn_tanh_backward(_p(ds), _p(s), _p(x), Cn, N, _p(mean), _p(invstd), _p(gamma), int(train), _p(dx), _p(dgamma),
                                            _p(dbeta), _stream(x.device)), "wg_mg_bn_tanh_backward")
    return dx


def mg_weight_norm(g, v):
    rows = v.size(0)
    w = torch.empty((rows, v[0].numel()), dtype=torch.float32, device=v.device)
    check(_lib.lib().wg_mg_weight_norm(_p(g), _p(v), rows, w.size(1), _p(w), _stream(v.device)), "wg_mg_weight_norm")
    return w


def mg_weight_norm_backward(g, v, dw):
    dg, dv = torch.empty_like(g), torch.empty_like(v)
    rows = v.size(0)
    check(_lib.lib().wg_mg_weight_norm_backward(_p(g), _p(v), _p(dw), rows, v[0].numel(), _p(dg), _p(dv), _stream(v.device)),
          "wg_mg_weight_norm_backward")
    return dg, dv


def lvc_check(dims, B, T, F):
    """0, or the library's error code for a shape its LVC kernels do not serve (wg_lvc_check; no launch, no device needed)."""
    return _lib.lib().wg_lvc_check(C.byref(dims), B, T, F)


def lvc_forward(dims, x, w, F):
    Bn, R, T = x.shape
    z = torch.empty((Bn, 2 * dims.dil_ch, T), dtype=torch.float32, device=x.device)
    gate = torch.empty((Bn, dims.dil_ch, T), dtype=torch.float32, device=x.device)
    check(_lib.lib().wg_lvc_forward(C.byref(dims), _p(x), _p(w), Bn, T, F, _p(z), _p(gate), _stream(x.device)), "wg_lvc_forward")
    return z, gate


def lvc_backward_data(dims, dz, w, F, dx_add=None):
    Bn, _, T = dz.shape
    dx = torch.empty((Bn, dims.res_ch, T), dtype=torch.float32, device=dz.device)
    check(_lib.lib().wg_lvc_backward_data(C.byref(dims), _p(dz), _p(w), _p(dx_add), Bn, T, F, _p(dx), _stream(dz.device)),
          "wg_lvc_backward_data")
    return dx


def lvc_backward_weight(dims, dz, x, F, out):
    Bn, _, T = dz.shape
    check(_lib.lib().wg_lvc_backward_weight(C.byref(dims), _p(dz), _p(x), Bn, T, F, _p(out), _stream(dz.device)), "wg_lvc_backward_weight")
    return out


def lvc_gate_backward(z, dgate):
    Bn, D, T = dgate.shape
    dz = torch.empty_like(z)
    check(_lib.lib().wg_lvc_gate_backward(_p(z), _p(dgate), Bn, D, T, _p(dz), _stream(z.device)), "wg_lvc_gate_backward")
    return dz


# ---- MelGlow's eval passes (include/wgflow.h wg_mg_check .. wg_mg_inverse; csrc/wg_mgflow.h) ------------------------------------------
class MelGlowEngine(_InverseGraphs):
    """Model-level, no-autograd passes of MelGlow in eval(): wg_mg_pack_weights once per weight change, then wg_mg_forward /
    wg_mg_inverse from the packed weights and one workspace.  `table`: the model's float state-dict tensors in the header's order."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.buffers = _Buffers()
        self.packed = PackedWeights()
        self._eps = None

    def check(self, B, N, F):
        """0, or the library's error code for a shape the passes do not serve (no launch, no device needed)."""
        return _lib.lib().wg_mg_check(C.byref(self.cfg), B, N, F)

    def _pack(self, table, eps, device):
        L = _lib.lib()
        if len(table) != L.wg_mg_param_count(C.byref(self.cfg)):
            raise WgError("MelGlow parameter table has %d entries, expected %d" % (len(table), L.wg_mg_param_count(C.byref(self.cfg))))
        eps = tuple(float(e) for e in eps)
        if self.packed.stale(table) or self.packed.buf.device != device or eps != self._eps:
            require_device(*table)
            nbytes = L.wg_mg_packed_bytes(C.byref(self.cfg))
            if nbytes == 0:
                raise WgError("MelGlow configuration not supported by the one-call passes (include/wgflow.h wg_mg_check)")
            if self.packed.buf is None or self.packed.buf.numel() < nbytes or self.packed.buf.device != device:
                self.packed.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            check(L.wg_mg_pack_weights(C.byref(self.cfg), _table([t.contiguous() if t is not None else None for t in table]),
                                       (C.c_float * len(eps))(*eps), _p(self.packed.buf), _stream()), "wg_mg_pack_weights")
            self.packed.commit()
            self._eps = eps
        return self.packed.buf

    def _launch(self, pk, ws, x, h, inverse):
        B, N = x.shape
        out = torch.empty_like(x)
        logdet = torch.empty(B, dtype=torch.float32, device=x.device)
        fn = _lib.lib().wg_mg_inverse if inverse else _lib.lib().wg_mg_forward
        check(fn(C.byref(self.cfg), _p(pk), _p(x), _p(h), B, N, h.shape[2], _p(out), _p(logdet), _p(ws), ws.numel(), _stream()),
              "wg_mg_inverse" if inverse else "wg_mg_forward")
        return out, logdet

    @on_device
    def run(self, x, h, table, eps, inverse, synthesis):
        """x [B, N] (N a multiple of the hop), h [B, n_mels, F >= N / hop]; inverse: reverse_computation.  synthesis: this is the
        direction towards the audio, which may be replayed from a captured graph (WG_GRAPHS, as ModelEngine.run)."""
        require_device(x, h)
        x, h = x.contiguous(), h.contiguous()
        B, N = x.shape
        pk = self._pack(table, eps, x.device)
        nbytes = _lib.lib().wg_mg_workspace_bytes(C.byref(self.cfg), B, N)
        ws = self.buffers.get((x.device, B, N), nbytes, x.device)
        if synthesis:
            key = (x.device, tuple(x.shape), h.shape[2], pk.data_ptr(), ws.data_ptr(), bool(inverse))
            return self._run_inverse(key, lambda sz, sh: self._launch(pk, ws, sz, sh, inverse), x, h)
        return self._launch(pk, ws, x, h, inverse)

    @on_device
    def predictor(self, h, table, eps, flow, frames=None):
        """Predictor.forward in eval() of flow `flow` through the passes' own launches: h [B, n_mels, F] -> [depth, B frames, 2D R radix]."""
        require_device(h)
        h = h.contiguous()
        B, _, F = h.shape
        Fr = F if frames is None else frames
        c = self.cfg
        pk = self._pack(table, eps, h.device)
        plane = (c.pred_ch * c.depth * B * Fr + 3) // 4 * 4
        ws = torch.empty(3 * plane, dtype=torch.float32, device=h.device)
        out = torch.empty((c.depth, B * Fr, 2 * c.dil_ch * c.res_ch * c.radix), dtype=torch.float32, device=h.device)
        check(_lib.lib().wg_mg_predictor_apply(C.byref(c), _p(pk), flow, _p(h), B, Fr, F, _p(out), _p(ws), ws.numel() * 4, _stream()),
              "wg_mg_predictor_apply")
        return out


def mg_layer_apply(dims, skip_ch, h, w, wo, F, skip, first, last):
    """One NonCausalLayerLVC in one launch (wg_mg_layer_apply): h [B, R, T], w [B, F, 2D, R, radix], wo the effective W_o [rows, D] ->
    (h + res in a new tensor, or None when last; skip stored (first) or added to in place)."""
    Bn, R, T = h.shape
    hn = None if last else torch.empty_like(h)
    check(_lib.lib().wg_mg_layer_apply(C.byref(dims), skip_ch, int(first), int(last), _p(h), _p(w), _p(wo), Bn, T, F, _p(hn), _p(skip),
                                       _stream(h.device)), "wg_mg_layer_apply")
    return hn, skip


# ---- MRWaveGlow's plumbing (csrc/wg_mr.h): one launch each, the caller's tensors in and out -------------------------------------------
def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def mr_haar_split(x, mode=0, cond_rows=0):
    """x [B, c, T] with any strides -> (diff, avg, cond): cond [B, cond_rows, T] (None when cond_rows is 0) has avg in its first rows."""
    Bn, c, T = x.shape
    diff, avg = _f32((Bn, c // 2, T), x), _f32((Bn, c // 2, T), x)
    cond = _f32((Bn, cond_rows, T), x) if cond_rows else None
    check(_lib.lib().wg_mr_haar_split(_p(x), x.stride(0), x.stride(1), x.stride(2), Bn, c, T, mode, _p(diff), _p(avg), _p(cond), cond_rows,
                                      _stream(x.device)), "wg_mr_haar_split")
    return diff, avg, cond


def mr_haar_merge(avg, diff, mode=0, channels_last=False, avg2=None):
    """(avg, diff) [B, c/2, T] -> [B, c, T], contiguous or (channels_last) as a view of a [B, T, c] tensor; avg2: rows of a
    [B, rows, T] tensor added to avg first."""
    Bn, half, T = avg.shape
    out = _f32((Bn, T, 2 * half), avg).transpose(1, 2) if channels_last else _f32((Bn, 2 * half, T), avg)
    check(_lib.lib().wg_mr_haar_merge(_p(avg), _p(avg2), 0 if avg2 is None else avg2.size(1), _p(diff), Bn, 2 * half, T, mode, _p(out),
                                      out.stride(0), out.stride(1), out.stride(2), _stream(avg.device)), "wg_mr_haar_merge")
    return out


def mr_upsample(h, s, T, out=None, r0=0, head=None):
    """h [B, n_mels, F] -> rows [r0, r0 + n_mels) of out [B, rows, T] (a new [B, r0 + n_mels, T] by default); head [B, r0, T] fills the
    rows before them."""
    Bn, n_mels, F = h.shape
    if out is None:
        out = _f32((Bn, r0 + n_mels, T), h)
    check(_lib.lib().wg_mr_upsample(_p(h), _p(head), Bn, n_mels, F, s, T, _p(out), out.size(1), r0, _stream(h.device)), "wg_mr_upsample")
    return out


def mr_upsample_backward(dout, r0, n_mels, F, s):
    Bn, rows, T = dout.shape
    dh = _f32((Bn, n_mels, F), dout)
    check(_lib.lib().wg_mr_upsample_backward(_p(dout), rows, r0, Bn, n_mels, F, s, T, _p(dh), _stream(dout.device)), "wg_mr_upsample_backward")
    return dh


def mr_pack(src, n_group, off, dst):
    """src [B, c, T] into channels [off, off + c) of the latent dst [B, T * n_group]"""
    Bn, c, T = src.shape
    check(_lib.lib().wg_mr_pack(_p(src), Bn, c, T, n_group, off, _p(dst), _stream(src.device)), "wg_mr_pack")
    return dst


def mr_unpack(src, n_group, off, c):
    """channels [off, off + c) of the latent src [B, T * n_group] -> [B, c, T]"""
    Bn, T = src.size(0), src.size(1) // n_group
    dst = _f32((Bn, c, T), src)
    check(_lib.lib().wg_mr_unpack(_p(src), Bn, c, T, n_group, off, _p(dst), _stream(src.device)), "wg_mr_unpack")
    return dst


# ---- MRWaveGlow's eval passes (include/wgflow.h wg_mr_check .. wg_mr_inverse) ----------------------------------------------------------
class MRWaveGlowEngine(_InverseGraphs):
    """Model-level, no-autograd passes of MRWaveGlow: wg_mr_pack_weights once per weight change, then wg_mr_forward / wg_mr_inverse
    from the packed weights and one zero-initialised workspace.  `params`: the model's state-dict tensors in the header's order."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.buffers = _Buffers()
        self.packed = PackedWeights()
        self.n_params = None

    def check(self, B, N, F):
        """0, or the library's error code for a call the passes do not serve (no launch, no device needed)."""
        return _lib.lib().wg_mr_check(C.byref(self.cfg), B, N, F)

    def _pack(self, params, device, key=None):
        L = _lib.lib()
        if self.n_params is None:
            self.n_params = L.wg_mr_param_count(C.byref(self.cfg))
        if len(params) != self.n_params:
            raise WgError("MRWaveGlow parameter table has %d entries, expected %d" % (len(params), self.n_params))
        if self.packed.stale(params, key) or self.packed.buf.device != device:
            require_device(*params)
            nbytes = L.wg_mr_packed_bytes(C.byref(self.cfg))
            if nbytes == 0:
                raise WgError("MRWaveGlow configuration not supported by the one-call passes (include/wgflow.h wg_mr_check)")
            if self.packed.buf is None or self.packed.buf.numel() < nbytes or self.packed.buf.device != device:
                self.packed.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            check(L.wg_mr_pack_weights(C.byref(self.cfg), _table([t.contiguous() if t is not None else None for t in params]),
                                       _p(self.packed.buf), _stream()), "wg_mr_pack_weights")
            self.packed.commit()
        return self.packed.buf

    def _launch(self, pk, ws, x, h, inverse):
        B, N = x.shape
        out = torch.empty_like(x)
        logdet = torch.empty(B, dtype=torch.float32, device=x.device)
        fn = _lib.lib().wg_mr_inverse if inverse else _lib.lib().wg_mr_forward
        check(fn(C.byref(self.cfg), _p(pk), _p(x), _p(h), B, N, h.shape[2], _p(out), _p(logdet), _p(ws), ws.numel(), _stream()),
              "wg_mr_inverse" if inverse else "wg_mr_forward")
        return out, logdet

    @on_device
    def run(self, params, x, h, inverse, key=None):
        """x [B, N], h [B, n_mels, F]; inverse: reverse_computation.  The pass towards the audio (reverse_computation, or
        forward_computation of a reverse_mode model) may be replayed from a captured graph (WG_GRAPHS, keyed as ModelEngine.run).
        `key`: PackedWeights.key_of(params), where the caller has it already."""
        require_device(x, h)
        x, h = x.contiguous(), h.contiguous()
        B, N = x.shape
        pk = self._pack(params, x.device, key)
        nbytes = _lib.lib().wg_mr_workspace_bytes(C.byref(self.cfg), B, N)
        ws = self.buffers.get((x.device, B, N), nbytes, x.device)
        if bool(inverse) != bool(self.cfg.reverse_mode):
            key = (x.device, tuple(x.shape), h.shape[2], pk.data_ptr(), ws.data_ptr(), bool(inverse))
            return self._run_inverse(key, lambda sz, sh: self._launch(pk, ws, sz, sh, inverse), x, h)
        return self._launch(pk, ws, x, h, inverse)
