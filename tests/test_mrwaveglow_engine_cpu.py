"""MRWaveGlow's one-call eval passes on the CPU side (no kernel launches): the C ABI's table order against the module tree, the size
queries, wg_mr_check against what MRWaveGlow's constructor and _check refuse, what wg_mr_forward / wg_mr_inverse answer before they
launch anything, and which calls MRWaveGlow routes to the engine."""
import ctypes as C
import os
import re

import pytest
import torch

import make_golden_mrwaveglow as mrg
import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import WgError, _lib

OK, EINVAL, ESHAPE, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -3, -5        # include/wgflow.h


def _cfg(arch=mrg.ARCH_SMALL, reverse_mode=False, super_resolution=False, precision=2, **over):
    kw = dict(levels=3, flows=4)
    kw.update(arch)
    kw.update(over)
    return _lib.WgMrConfig(kw["prior_flows"], kw["flows"], kw["levels"], kw["n_group"], kw["hop_size"], kw["n_mels"], int(super_resolution),
                           int(reverse_mode), kw["dilation_channels"], kw["residual_channels"], kw["skip_channels"], kw["depth"], kw["radix"],
                           int(kw["bias"]), precision)


def _check(cfg, B, N, F):
    return _lib.lib().wg_mr_check(C.byref(cfg), B, N, F)


def test_param_count_at_the_shipped_config():
    assert _lib.lib().wg_mr_param_count(C.byref(_cfg(mrg.ARCH_FULL))) == 456       # 456 state-dict entries


ARCHS = {"shipped": (mrg.ARCH_FULL, False), "mr_small": (mrg.ARCH_SMALL, False), "mr_small_sr": (mrg.ARCH_SMALL, True),
         "mr_ragged": (mrg.ARCH_RAGGED, False), "bias": (dict(mrg.ARCH_SMALL, bias=True), False)}


@pytest.mark.parametrize("name", list(ARCHS))
def test_table_is_the_state_dict_in_order(name, monkeypatch):
    monkeypatch.delenv("WG_PRECISION", raising=False)
    arch, sr = ARCHS[name]
    m = cm.MRWaveGlow(memory_efficient=True, super_resolution=sr, **arch)
    want = list(m.state_dict(keep_vars=True).items())
    table = m.mr_table()
    assert len(table) == len(want) == _lib.lib().wg_mr_param_count(C.byref(m.mr_config()))
    for t, (k, v) in zip(table, want):
        assert t is v, k
    cfg, want_cfg = m.mr_config(), _cfg(arch, super_resolution=sr)
    assert [getattr(cfg, n) for n, _ in cfg._fields_] == [getattr(want_cfg, n) for n, _ in cfg._fields_]
    # weight norm removed: a conv keeps its two slots, the first one empty (a NULL weight_g); what is left is the state dict in order
    m.apply(cm.remove_weight_norms)
    table = m.mr_table()
    assert len(table) == len(want)
    left = list(m.state_dict(keep_vars=True).items())
    assert not any(k.endswith("weight_g") for k, _ in left)
    filled = [t for t in table if t is not None]
    assert len(filled) == len(left) and all(t is v for t, (_, v) in zip(filled, left))
    gaps = [i for i, t in enumerate(table) if t is None]
    assert len(gaps) == sum(k.endswith("weight_g") for k, _ in want) and all(want[i][0].endswith("weight_g") for i in gaps)


def test_config_mirror_matches_the_header():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wgflow.h")).read()
    body = re.search(r"typedef struct wg_mr_config \{(.*?)\} wg_mr_config;", header, re.S).group(1)
    names = [n.strip() for decl in re.findall(r"int32_t([^;]*);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _lib.WgMrConfig._fields_]


def test_sizes_are_nonzero_and_constant_in_flow_count():
    L = _lib.lib()
    cfg = _cfg(mrg.ARCH_FULL)
    assert L.wg_mr_packed_bytes(C.byref(cfg)) > 53_735_520 * 4 - 12 * 8 * 8 * 4          # every WN weight in at least one layout
    w = lambda c, B, N: int(L.wg_mr_workspace_bytes(C.byref(c), B, N))
    w12 = w(cfg, 24, 16000)
    w3 = w(_cfg(mrg.ARCH_FULL, prior_flows=1, flows=1), 24, 16000)
    assert 0 < w3 <= w12 <= 2 * w3                             # O(1) in flow count apart from the partial slab
    assert 0 < w(cfg, 1, 62 * 256) < w(cfg, 2, 62 * 256) < w(cfg, 1, 860 * 256)
    assert w(cfg, 24, 16001) == 0 and w(cfg, 0, 256) == 0 and w(cfg, 1, 0) == 0         # N % n_group, no item, no audio
    assert L.wg_mr_packed_bytes(None) == 0 and L.wg_mr_workspace_bytes(None, 1, 256) == 0 and L.wg_mr_check(None, 1, 256, 1) == EINVAL
    assert L.wg_mr_param_count(None) == 0


# what the kernels (or the constructor) refuse: code, and whether MRWaveGlow(...) itself raises for it
REFUSED = [
    (dict(residual_channels=250), EUNSUPPORTED, False),        # channels no multiple of 32
    (dict(radix=4), EUNSUPPORTED, False),                      # even kernel
    (dict(n_group=12, hop_size=240), EINVAL, True),            # 12 -> 6 -> 3: odd after levels - 1 halvings
    (dict(n_group=8, levels=4), EINVAL, True),                 # 8 is no multiple of 2^4
    (dict(n_group=8, hop_size=4), EINVAL, True),               # a frame owns no column
    (dict(n_group=64, hop_size=256), EUNSUPPORTED, False),     # the 1x1 mixes at most 32 channels
    (dict(prior_flows=0, flows=0), EUNSUPPORTED, False),       # no flow at all
    (dict(prior_flows=0, levels=1, n_group=8), EUNSUPPORTED, False),
    (dict(prior_flows=40, flows=13), EUNSUPPORTED, False),     # 66 flows
    (dict(depth=17), EINVAL, False),                           # (what wn_check answers for a depth outside 1 .. 16)
]


@pytest.mark.parametrize("over,code,ctor_raises", REFUSED)
def test_refused_configurations_answer_without_a_launch(over, code, ctor_raises):
    L = _lib.lib()
    cfg = _cfg(**over)
    frames = 8
    N = frames * cfg.hop_size // cfg.n_group * cfg.n_group if cfg.hop_size >= cfg.n_group else 64
    before = L.wg_stat_mr_pass_calls()
    assert _check(cfg, 2, N, frames) == code
    assert L.wg_mr_packed_bytes(C.byref(cfg)) == 0 and L.wg_mr_workspace_bytes(C.byref(cfg), 2, N) == 0 and L.wg_mr_param_count(C.byref(cfg)) == 0
    p, null = C.c_void_p(4096), C.c_void_p(0)
    for fn in (L.wg_mr_forward, L.wg_mr_inverse):
        assert fn(C.byref(cfg), p, p, p, 2, N, frames, p, p, p, 1 << 40, null) == code
    assert L.wg_mr_pack_weights(C.byref(cfg), p, p, null) == code
    assert L.wg_stat_mr_pass_calls() == before
    kw = dict(levels=3, flows=4)
    kw.update(mrg.ARCH_SMALL)
    kw.update(over)
    if ctor_raises:                                            # the check agrees with the constructor
        with pytest.raises(WgError):
            cm.MRWaveGlow(memory_efficient=True, **kw)
    elif kw["depth"] <= 16 and kw["prior_flows"] + kw["flows"] < 40:
        m = cm.MRWaveGlow(memory_efficient=True, **kw).eval()  # a valid model: its calls take the module path
        with torch.no_grad():
            assert "wg_mr_check: code %d" % code == m._engine_route(torch.zeros(2, N), torch.zeros(2, kw["n_mels"], frames))[0]


def test_shapes_and_workspace_are_answered_before_any_launch():
    """Dummy non-NULL addresses: none of these paths dereferences or launches anything (no device in this process)."""
    L = _lib.lib()
    cfg = _cfg()
    m = cm.MRWaveGlow(memory_efficient=True, **mrg.ARCH_SMALL)
    before = L.wg_stat_mr_pass_calls()
    assert _check(cfg, 2, 8 * 256, 8) == OK and _check(cfg, 2, 8 * 256, 11) == OK       # extra trailing frames are allowed
    assert _check(cfg, 2, 8 * 256 - 8, 8) == OK                                         # ... and an audio cut short of them
    assert _check(cfg, 2, 8 * 256 + 3, 9) == ESHAPE                                     # N % n_group
    assert _check(cfg, 2, 8 * 256 + 8, 8) == ESHAPE                                     # T > F s
    assert _check(cfg, 0, 256, 1) == EINVAL and _check(cfg, 1, 256, 0) == EINVAL
    assert _check(cfg, 65535, 8, 1) == OK and _check(cfg, 65536, 8, 1) == EUNSUPPORTED  # items are a grid axis
    assert _check(_cfg(precision=3), 2, 8 * 256, 8) == EINVAL
    # ... and MRWaveGlow._check raises for the same shapes before it looks at the device
    for N, F in ((8 * 256 + 3, 9), (8 * 256 + 8, 8)):
        with pytest.raises(WgError, match="multiple of n_group|upsample to"):
            m._check(torch.zeros(2, N), torch.zeros(2, 80, F))
    p, null = C.c_void_p(4096), C.c_void_p(0)
    need = int(L.wg_mr_workspace_bytes(C.byref(cfg), 2, 8 * 256))
    for fn in (L.wg_mr_forward, L.wg_mr_inverse):
        call = lambda N=8 * 256, F=8, ws=p, n=need, x=p: fn(C.byref(cfg), p, x, p, 2, N, F, p, p, ws, n, null)
        assert call(n=need - 1) == EWORKSPACE and call(n=0) == EWORKSPACE
        assert call(N=8 * 256 + 3, F=9) == ESHAPE and call(N=8 * 256 + 8) == ESHAPE
        assert call(ws=null) == EINVAL and call(x=null) == EINVAL
    assert L.wg_mr_pack_weights(C.byref(cfg), None, p, null) == EINVAL
    n = L.wg_mr_param_count(C.byref(cfg))
    table = (C.c_void_p * n)(*([4096] * n))
    table[cfg.prior_flows + 1] = None                                                   # a weight_v may not be absent
    assert L.wg_mr_pack_weights(C.byref(cfg), table, p, null) == EINVAL
    table[cfg.prior_flows + 1] = 4096
    table[0] = None                                                                     # nor a 1x1 weight
    assert L.wg_mr_pack_weights(C.byref(cfg), table, p, null) == EINVAL
    assert L.wg_stat_mr_pass_calls() == before


def test_edge_configurations_the_check_serves():
    """levels == 1 and prior_flows == 0 are served as long as a flow is left; flows == 0 with prior flows too."""
    for over in (dict(levels=1), dict(prior_flows=0), dict(flows=0), dict(levels=2), dict(n_group=32, levels=5, hop_size=256)):
        cfg = _cfg(**over)
        N = 4 * cfg.hop_size
        assert _check(cfg, 1, N, 4) == OK, over
        assert _lib.lib().wg_mr_workspace_bytes(C.byref(cfg), 1, N) > 0 and _lib.lib().wg_mr_packed_bytes(C.byref(cfg)) > 0
        kw = dict(mrg.ARCH_SMALL)
        kw.update(over)
        m = cm.MRWaveGlow(memory_efficient=True, **kw)
        assert len(m.mr_table()) == _lib.lib().wg_mr_param_count(C.byref(cfg)) == len(m.state_dict())


def test_routing_predicate_on_cpu_tensors(monkeypatch):
    """Which calls go to the engine is decided before any tensor is touched.  train() or grad enabled: the module path, with today's
    error for CPU tensors; in eval() under no_grad everything but the device holds for CPU tensors, and the module path answers too."""
    monkeypatch.delenv("WG_MR_ENGINE", raising=False)
    m = cm.MRWaveGlow(memory_efficient=True, **mrg.ARCH_SMALL)
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
        assert why() == "tensors are not float32 on one HIP device"                     # CPU tensors
        assert m._engine_route(x.half(), h.half())[0] == "tensors are not float32 on one HIP device"       # half tensors
        assert m._engine_route(x.double(), h)[0] == "tensors are not float32 on one HIP device"
        assert "not audio" in m._engine_route(x[0], h)[0]
        assert "wg_mr_check: code %d" % ESHAPE == m._engine_route(torch.zeros(2, 8 * 256 + 3), h)[0]
        m.prior_WNs[1].train()                                                          # one block left in train()
        assert "train()" in why()
        m.eval()
        monkeypatch.setenv("WG_MR_ENGINE", "0")
        assert why() == "WG_MR_ENGINE=0"
        monkeypatch.setenv("WG_MR_ENGINE", "1")
        assert why() == "tensors are not float32 on one HIP device"
        m.half()
        assert why() == "parameters are not float32"
