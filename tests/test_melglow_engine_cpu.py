"""MelGlow's one-call eval passes on the CPU side (no kernel launches): the C ABI's table order against the module tree, the size
queries, wg_mg_check on both sides of each of its limits, what wg_mg_forward / wg_mg_inverse answer before they launch anything, and
which calls MelGlow routes to the engine."""
import ctypes as C

import pytest
import torch

import make_golden_melglow as mgg
import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import WgError, _lib

OK, EINVAL, ESHAPE, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -3, -5        # include/wgflow.h


def _cfg(arch=mgg.ARCH_SMALL, reverse_mode=False, **over):
    kw = dict(arch)
    kw.update(over)
    return _lib.WgMgConfig(kw["flows"], kw["n_group"], kw["n_early_every"], kw["n_early_size"], kw["hop_size"], kw["n_mels"], kw["depth"],
                           kw["residual_channels"], kw["dilation_channels"], kw["skip_channels"], kw["radix"], kw["predict_channels"],
                           kw["predict_layers"], int(reverse_mode))


def _check(cfg, B, N, F):
    return _lib.lib().wg_mg_check(C.byref(cfg), B, N, F)


@pytest.mark.parametrize("arch", [mgg.ARCH_SMALL, mgg.ARCH_RAGGED, mgg.ARCH_FULL], ids=["small", "ragged", "full"])
def test_table_is_the_float_state_dict_in_order(arch):
    m = cm.MelGlow(memory_efficient=True, **arch)
    want = [(k, v) for k, v in m.state_dict(keep_vars=True).items() if v.is_floating_point()]
    skipped = [k for k, v in m.state_dict().items() if not v.is_floating_point()]
    assert skipped and all(k.endswith("num_batches_tracked") for k in skipped)
    table = m.mg_table()
    assert len(table) == len(want) == _lib.lib().wg_mg_param_count(C.byref(m.mg_config()))
    for t, (k, v) in zip(table, want):
        assert t is v, k
    cfg, want_cfg = m.mg_config(), _cfg(arch)
    assert [getattr(cfg, n) for n, _ in cfg._fields_] == [getattr(want_cfg, n) for n, _ in cfg._fields_]
    # weight norm removed: a conv keeps its two slots, the first one empty (a NULL weight_g)
    m.apply(cm.remove_weight_norms)
    table = m.mg_table()
    assert len(table) == len(want)
    assert table[arch["flows"]] is None and table[arch["flows"] + 1] is m.WNs[0].F.start.weight
    assert table[arch["flows"] + 2] is None and table[arch["flows"] + 3] is m.WNs[0].F.layers[0].W_o.weight


def test_config_mirror_matches_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wgflow.h")).read()
    body = re.search(r"typedef struct wg_mg_config \{(.*?)\} wg_mg_config;", header, re.S).group(1)
    names = [n.strip() for decl in re.findall(r"int32_t([^;]*);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _lib.WgMgConfig._fields_]


def test_sizes_are_nonzero_inside_the_limits_and_grow():
    L = _lib.lib()
    cfg = _cfg(mgg.ARCH_FULL)
    assert L.wg_mg_packed_bytes(C.byref(cfg)) > 77_260_688 * 4 - 12 * 48 * 8                  # every weight once (weight_g folded in)
    w = lambda B, N: int(L.wg_mg_workspace_bytes(C.byref(cfg), B, N))
    assert 0 < w(1, 62 * 256) < w(2, 62 * 256) < w(8, 62 * 256)
    assert w(1, 62 * 256) < w(1, 63 * 256) < w(1, 860 * 256)
    assert w(1, 62 * 256 + 8) == 0 and w(0, 256) == 0 and w(1, 0) == 0                        # N % hop, no item, no audio
    assert L.wg_mg_packed_bytes(C.byref(_cfg(radix=2))) == 0 and L.wg_mg_param_count(C.byref(_cfg(radix=2))) == 0
    assert L.wg_mg_packed_bytes(None) == 0 and L.wg_mg_workspace_bytes(None, 1, 256) == 0 and L.wg_mg_check(None, 1, 256, 1) == EINVAL


@pytest.mark.parametrize("over,B,frames,want", [
    (dict(), 1, 4, OK),
    (dict(dilation_channels=64), 1, 4, OK), (dict(dilation_channels=65), 1, 4, EUNSUPPORTED),               # D L: 2048 / 2080 at L = 32
    (dict(residual_channels=64), 1, 4, OK), (dict(residual_channels=65), 1, 4, EUNSUPPORTED),               # R L
    (dict(residual_channels=85, hop_size=64), 1, 4, OK), (dict(residual_channels=86, hop_size=64), 1, 4, EUNSUPPORTED),   # R radix: 255 / 258
    (dict(hop_size=1024, dilation_channels=4, residual_channels=4), 1, 4, OK),                               # L = 128
    (dict(hop_size=1032, dilation_channels=4, residual_channels=4), 1, 4, EUNSUPPORTED),                     # L = 129
    (dict(hop_size=260), 1, 4, EUNSUPPORTED),                                                                # hop not a multiple of n_group
    (dict(radix=5), 1, 4, OK), (dict(radix=4), 1, 4, EUNSUPPORTED),                                          # even kernel
    (dict(n_group=32, n_early_size=2), 1, 4, OK), (dict(n_group=34, n_early_size=2, hop_size=272), 1, 4, EUNSUPPORTED),   # the 1x1 mixes <= 32 channels
    (dict(n_early_size=1), 1, 4, EUNSUPPORTED),                                                              # 7 channels in flows 2, 3: no halves
    (dict(flows=64, n_early_every=64), 1, 4, OK), (dict(flows=65, n_early_every=65), 1, 4, EUNSUPPORTED),
    (dict(depth=16), 1, 4, OK), (dict(depth=17), 1, 4, EUNSUPPORTED),
    (dict(skip_channels=4096), 1, 4, OK), (dict(skip_channels=4097), 1, 4, EUNSUPPORTED),
    (dict(predict_channels=4096), 1, 4, OK), (dict(predict_channels=4097), 1, 4, EUNSUPPORTED),
    (dict(), 65535, 1, OK), (dict(), 65536, 1, EUNSUPPORTED),                                                # items are a grid axis
    (dict(), 1, 65535 * 64, OK), (dict(), 1, 65535 * 64 + 1, EUNSUPPORTED),                                  # B frames: the end product's row tiles
    (dict(flows=0), 1, 4, EINVAL), (dict(predict_layers=-1), 1, 4, EINVAL), (dict(predict_layers=0), 1, 4, OK),
])
def test_check_limits_on_both_sides(over, B, frames, want):
    cfg = _cfg(**over)
    assert _check(cfg, B, frames * cfg.hop, frames) == want
    if want in (EUNSUPPORTED, EINVAL):
        assert _lib.lib().wg_mg_workspace_bytes(C.byref(cfg), B, frames * cfg.hop) == 0


def test_shapes_and_workspace_are_answered_before_any_launch():
    """Dummy non-NULL addresses: none of these paths dereferences or launches anything (no device in this process)."""
    L = _lib.lib()
    cfg = _cfg()
    before = (L.wg_stat_mg_pass_calls(), L.wg_stat_mg_layer_launches())
    assert _check(cfg, 2, 8 * 256, 8) == OK and _check(cfg, 2, 8 * 256, 11) == OK       # extra trailing frames are allowed
    assert _check(cfg, 2, 8 * 256 + 8, 9) == ESHAPE                                     # N % hop
    assert _check(cfg, 2, 8 * 256, 7) == ESHAPE                                         # F < N / hop
    assert _check(cfg, 0, 256, 1) == EINVAL and _check(cfg, 1, 256, 0) == EINVAL
    p, null = C.c_void_p(4096), C.c_void_p(0)
    need = int(L.wg_mg_workspace_bytes(C.byref(cfg), 2, 8 * 256))
    for fn in (L.wg_mg_forward, L.wg_mg_inverse):
        call = lambda N=8 * 256, F=8, ws=p, n=need, x=p: fn(C.byref(cfg), p, x, p, 2, N, F, p, p, ws, n, null)
        assert call(n=need - 1) == EWORKSPACE and call(n=0) == EWORKSPACE
        assert call(N=8 * 256 + 8, F=9) == ESHAPE and call(F=7) == ESHAPE
        assert call(ws=null) == EINVAL and call(x=null) == EINVAL
        assert fn(C.byref(_cfg(radix=4)), p, p, p, 2, 8 * 256, 8, p, p, p, 1 << 40, null) == EUNSUPPORTED
    assert L.wg_mg_pack_weights(C.byref(cfg), None, None, p, null) == EINVAL
    n = L.wg_mg_param_count(C.byref(cfg))
    table = (C.c_void_p * n)(*([4096] * n))
    table[cfg.flows + 1] = None                                                         # a weight_v may not be absent
    assert L.wg_mg_pack_weights(C.byref(cfg), table, None, p, null) == EINVAL
    assert (L.wg_stat_mg_pass_calls(), L.wg_stat_mg_layer_launches()) == before


def test_routing_predicate_on_cpu_tensors():
    """Which calls go to the engine is decided before any tensor is touched.  train() or grad enabled: the module path, with today's
    error for CPU tensors; in eval() under no_grad everything but the device holds for CPU tensors, and the module path answers too."""
    m = cm.MelGlow(memory_efficient=True, **mgg.ARCH_SMALL)
    x, h = torch.zeros(2, 8 * 256), torch.zeros(2, 80, 8)
    why = lambda: m._engine_route(x, h)[0]
    assert "autograd" in why()                                                          # train() + grad
    with torch.no_grad():
        assert "train()" in why()
    m.eval()
    assert "autograd" in why()
    for ctx in (torch.enable_grad, torch.no_grad):
        with ctx(), pytest.raises(WgError, match="no CPU fallback"):
            m(x, h)
    with torch.no_grad():
        assert why() == "tensors are not float32 on one HIP device"
        assert "not audio" in m._engine_route(x[0], h)[0]
        m.WNs[1].F.pred.start[1].train()                                                # one BatchNorm left in train(): its statistics must move
        assert "train()" in why()
        m.eval()
        m.WNs[2].F.pred.res_blocks[0][4] = torch.nn.BatchNorm1d(m.WNs[2].F.pred.res_blocks[0][4].num_features, affine=False).eval()
        assert "BatchNorm" in why()
    m2 = cm.MelGlow(memory_efficient=True, **mgg.ARCH_SMALL).eval()
    with torch.no_grad():
        import os
        os.environ["WG_MG_ENGINE"] = "0"
        try:
            assert m2._engine_route(x, h)[0] == "WG_MG_ENGINE=0"
        finally:
            del os.environ["WG_MG_ENGINE"]
        assert "wg_mg_check" in m2._engine_route(torch.zeros(2, 255), h)[0]             # less than one frame of audio
        assert m2._engine_route(x.double(), h)[0] == "tensors are not float32 on one HIP device"
