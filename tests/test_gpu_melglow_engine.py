"""MelGlow's one-call eval passes on the MI355X (-m gpu): wg_mg_forward / wg_mg_inverse behind MelGlow.forward / reverse / infer in eval()
under no_grad, against the reference's own eval inverse (tests/golden/mg/), against the module path of the same model, the layer kernel
and the predictor's BatchNorm epilogue on their own against the float64 restatements of golden/mg_ref64.py, run-to-run and
graph-replay identity, and the calls that must stay on the module path.

Bars (those of test_gpu_melglow.py): x / z 1e-4 abs, logdet rtol 1e-4 with atol 1e-7 per sample, round-trip logdet 1e-3, the layer and
the predictor 1e-5 of the tensor's max-abs."""
import os

import numpy as np
import pytest
import torch

import fill
import make_golden_melglow as mgg
from mg_ref64 import LAYER_SHAPES, layer64, lvc_inputs, predictor64, shape_id
import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import _lib, engine, melglow

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mg")
Z_ATOL = 1e-4


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def stats():
    L = _lib.lib()
    return L.wg_stat_mg_pass_calls(), L.wg_stat_mg_layer_launches()


_CASES = {}


def case(name):
    """(model in eval() with the fixture's post-step running statistics, arch, fixture, h, z): built once per fixture, never modified"""
    if name not in _CASES:
        arch, tag, me, rmode = mgg.CASES[name]
        ref = np.load(os.path.join(GOLD, "model_%s.npz" % name))
        m = cm.MelGlow(memory_efficient=me, reverse_mode=rmode, **arch)
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(m, tag, arch).items()}
        for k in sd:
            sd[k] = torch.from_numpy(ref["buf::" + k]) if "buf::" + k in ref.files else sd[k]
        m.load_state_dict(sd)
        B, N = mgg.SHAPES[mgg.INPUT_TAG[name]]
        _, h = mgg.inputs(mgg.INPUT_TAG[name], B, N, arch["n_mels"], arch["hop_size"])
        _CASES[name] = (m.to(DEV).eval(), arch, ref, torch.from_numpy(h).to(DEV), torch.from_numpy(ref["z"]).to(DEV))
    return _CASES[name]


@pytest.fixture
def graphs_off(monkeypatch):
    monkeypatch.setenv("WG_GRAPHS", "0")
    monkeypatch.delenv("WG_MG_ENGINE", raising=False)


def check_logdet(got, want, size):
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-7 * size)


# ---- against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mg_small", "mg_small_nme", "mg_small_rm", "mg_ragged"])
def test_eval_inverse_vs_reference_and_back(name, graphs_off):
    m, arch, ref, h, z = case(name)
    keep = z.clone()
    c0, l0 = stats()
    with torch.no_grad():
        x, ld = m.reverse(z, h)
    c1, l1 = stats()
    assert c1 - c0 == 1 and l1 - l0 == arch["flows"] * arch["depth"]
    assert torch.equal(z, keep)
    assert float((x.cpu() - torch.from_numpy(ref["x_inv_eval"])).abs().max()) < Z_ATOL
    check_logdet(ld, ref["logdet_inv_eval"], ref["z"].size)
    # the other direction on the fixture's own x: the fixture's z, and the two logdets cancel
    xin = torch.from_numpy(ref["x_inv_eval"]).to(DEV)
    with torch.no_grad():
        z2, ld2 = m(xin, h)
    assert stats()[0] - c1 == 1
    assert float((z2.cpu() - torch.from_numpy(ref["z"])).abs().max()) < 1e-4
    assert float((ld2.cpu() + torch.from_numpy(ref["logdet_inv_eval"])).abs().max()) < 1e-3


@pytest.mark.parametrize("name", ["mg_small", "mg_ragged"])
def test_same_model_both_paths(name, monkeypatch):
    m, arch, ref, h, z = case(name)
    monkeypatch.setenv("WG_GRAPHS", "0")
    keep = z.clone()
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("WG_MG_ENGINE", flag)
        c0 = stats()[0]
        with torch.no_grad():
            out[flag] = m.reverse(z, h)
        assert stats()[0] - c0 == int(flag)
        assert torch.equal(z, keep)
        assert float((out[flag][0].cpu() - torch.from_numpy(ref["x_inv_eval"])).abs().max()) < Z_ATOL
        check_logdet(out[flag][1], ref["logdet_inv_eval"], ref["z"].size)
    dx = float((out["0"][0] - out["1"][0]).abs().max())
    dl = float((out["0"][1] - out["1"][1]).abs().max())
    print("%s: module path vs engine: max |dx| %.3e, max |dlogdet| %.3e" % (name, dx, dl))
    assert dx < 2 * Z_ATOL, "module path vs engine: max |dx| %.3e, max |dlogdet| %.3e" % (dx, dl)


# ---- the layer kernel alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=shape_id)
def test_layer_kernel_vs_float64(shape):
    R, D, S, radix, L, F, B, dilation, last = shape
    xn, wn = lvc_inputs("klayer/%d" % dilation, R, D, radix, L, F, B)
    h, w = torch.from_numpy(xn).to(DEV), torch.from_numpy(wn).to(DEV)
    rows = S if last else R + S
    wo = torch.from_numpy(fill.normal("mgl/wo%d" % dilation, (rows, D), 1.0 / np.sqrt(D))).to(DEV)
    wo2 = torch.from_numpy(fill.normal("mgl/wo2%d" % dilation, (rows, D), 1.0 / np.sqrt(D))).to(DEV)
    dims = _lib.WgLvcDims(R, D, radix, dilation)
    keep = h.clone()
    skip = torch.full((B, S, F * L), float("nan"), device=DEV)
    l0 = stats()[1]
    hn, _ = engine.mg_layer_apply(dims, S, h, w, wo, F, skip, first=True, last=last)
    r64, s64 = layer64(h.double(), w.double(), dilation, wo.double(), R, last)
    assert torch.equal(h, keep)                                       # h_next is another buffer: the neighbours' halo stays intact
    assert rel(skip, s64) < 1e-5
    if last:
        assert hn is None
    else:
        assert hn.data_ptr() != h.data_ptr() and rel(hn, r64) < 1e-5
    # a second layer adds its skip in place (and reads the first one's h + res, or h again behind a last layer)
    h2 = h if last else hn
    keep2 = h2.clone()
    hn2, _ = engine.mg_layer_apply(dims, S, h2, w, wo2, F, skip, first=False, last=last)
    r64b, s64b = layer64(h2.double(), w.double(), dilation, wo2.double(), R, last)
    assert stats()[1] - l0 == 2
    assert torch.equal(h2, keep2)
    assert rel(skip, s64 + s64b) < 1e-5
    if not last:
        assert rel(hn2, r64b) < 1e-5


# ---- the predictor's BatchNorm epilogue --------------------------------------------------------------------------------------------
def test_eval_predictor_vs_float64_with_a_large_running_mean():
    arch = dict(mgg.ARCH_RAGGED, predict_layers=2, predict_channels=6)
    m = cm.MelGlow(memory_efficient=True, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(m, "mge/", arch).items()})
    flow = 1
    pred = m.WNs[flow].F.pred
    # A BatchNorm with running mean ~1000 and unit variance behind a product that is ~1000 + O(1).  So that the float64 yardstick sees
    # the same activation, that product is exact in float32: h and the start conv's weight are multiples of 1/8 and 1/16 (every partial
    # sum fits 24 bits in any order), and a constant mel channel carries the 1000.
    B, F, Fr = 3, 7, 5                         # two trailing frames that must not be read
    hq = np.clip(np.round(fill.normal("mge/h", (B, 80, F)) * 8) / 8, -2, 2).astype(np.float32)
    hq[:, 79] = 1.0
    with torch.no_grad():
        w0 = pred.start[0].weight
        w0.copy_(torch.from_numpy(np.round(fill.uniform("mge/w0", tuple(w0.shape), -0.25, 0.25) * 16) / 16))
        w0[:, 79] = 1000.0
        bn = pred.start[1]
        bn.running_mean.copy_(1000.0 + torch.from_numpy(fill.uniform("mge/rm", (bn.num_features,), -0.1, 0.1)))
        bn.running_var.fill_(1.0)
    ref = melglow.Predictor(80, 2 * arch["dilation_channels"] * arch["residual_channels"] * arch["radix"], 6, 2, False, arch["depth"])
    ref.load_state_dict(pred.state_dict())
    ref = ref.double().to(DEV)
    m = m.to(DEV).eval()
    h = torch.from_numpy(hq).to(DEV)
    eps = [b.eps for b in m.modules() if isinstance(b, torch.nn.BatchNorm1d)]
    before = [b.clone() for b in m.buffers()]
    out = m.mg_engine().predictor(h, [t.detach() for t in m.mg_table()], eps, flow, frames=Fr)
    o64, _ = predictor64(ref, h[..., :Fr].double(), False)             # [B, G M, Fr]
    G = arch["depth"]
    want = o64.reshape(B, G, -1, Fr).permute(1, 0, 3, 2).reshape(G, B * Fr, -1)
    assert out.shape == want.shape
    assert float(want.abs().max()) > 1e-2
    assert rel(out, want) < 1e-5
    assert all(torch.equal(a, b) for a, b in zip(before, m.buffers()))
    # and against the module path's eval predictor (three launches per BatchNorm): the same values to rounding
    with torch.no_grad():
        mod = m.WNs[flow].F.pred(h[..., :Fr].contiguous())
    assert rel(mod.reshape(B, G, -1, Fr).permute(1, 0, 3, 2).reshape(G, B * Fr, -1), want) < 1e-5


# ---- determinism and graphs --------------------------------------------------------------------------------------------------------
def test_bit_identical_runs_graph_replay_and_repack(monkeypatch):
    arch, tag, me, rmode = mgg.CASES["mg_small"]
    m0, _, ref, h, z = case("mg_small")
    m = cm.MelGlow(memory_efficient=me, reverse_mode=rmode, **arch)
    m.load_state_dict(m0.state_dict())
    m = m.to(DEV).eval()
    monkeypatch.delenv("WG_MG_ENGINE", raising=False)

    def run(graphs):
        monkeypatch.setenv("WG_GRAPHS", graphs)
        _lib.lib().wg_reload_env()
        with torch.no_grad():
            return m.reverse(z, h)

    a, b = run("0"), run("0")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c0 = stats()[0]
    g1, g2 = run("1"), run("1")                                        # captured, then replayed
    assert len(m.mg_engine()._graphs) == 1
    assert stats()[0] - c0 == 2                                        # the warm-up and the capture; a replay calls nothing
    for g in (g1, g2):
        assert torch.equal(g[0], a[0]) and torch.equal(g[1], a[1])
    with torch.no_grad():                                              # an in-place weight change: re-packed into the same buffer
        m.WNs[1].F.end.weight.mul_(1.5)
        m.WNs[2].F.pred.start[1].running_mean.add_(0.05)
        m.invconv1x1[0].weight.mul_(1.1)
    g3 = run("1")
    assert len(m.mg_engine()._graphs) == 1 and stats()[0] - c0 == 2
    d = run("0")
    assert not torch.equal(d[0], a[0])
    assert torch.equal(g3[0], d[0]) and torch.equal(g3[1], d[1])
    monkeypatch.setenv("WG_MG_ENGINE", "0")
    with torch.no_grad():
        mod = m.reverse(z, h)
    assert float((mod[0] - d[0]).abs().max()) < Z_ATOL
    check_logdet(d[1], mod[1].cpu().numpy(), z.numel())


# ---- what stays on the module path -------------------------------------------------------------------------------------------------
def test_fallbacks_keep_the_module_path(graphs_off):
    arch, tag, me, rmode = mgg.CASES["mg_small"]
    m0, _, ref, h, z = case("mg_small")
    m = cm.MelGlow(memory_efficient=me, reverse_mode=rmode, **arch)
    m.load_state_dict(m0.state_dict())
    m = m.to(DEV)
    B, N = z.shape
    hop = arch["hop_size"]
    # train() + infer: the running statistics keep moving, as upstream
    m.train()
    c0 = stats()[0]
    nbt = int(m.WNs[0].F.pred.start[1].num_batches_tracked)
    out = m.infer(h, sigma=0.6)
    assert stats()[0] == c0 and int(m.WNs[0].F.pred.start[1].num_batches_tracked) == nbt + 1
    assert out.shape == (B, h.size(2) * hop)
    # eval() with grad enabled: the module path (its outputs carry a graph)
    m.eval()
    zz, ld = m(torch.from_numpy(ref["x_inv_eval"]).to(DEV), h)
    assert stats()[0] == c0 and ld.requires_grad
    # extra trailing frames and a ragged audio tail: the engine gives the module path's shapes and values
    h_long = torch.cat((h, torch.from_numpy(fill.normal("mge/tail", (B, arch["n_mels"], 3))).to(DEV)), 2)
    z_long = torch.cat((z, torch.from_numpy(fill.normal("mge/ztail", (B, hop - 8))).to(DEV)), 1)
    keep = z_long.clone()
    with torch.no_grad():
        x1, l1 = m.reverse(z_long, h_long)
        assert stats()[0] == c0 + 1
        os.environ["WG_MG_ENGINE"] = "0"
        try:
            x0, l0 = m.reverse(z_long, h_long)
        finally:
            del os.environ["WG_MG_ENGINE"]
        x2, _ = m.reverse(z, h)
    assert stats()[0] == c0 + 2
    assert torch.equal(z_long, keep)
    assert x1.shape == x0.shape == (B, N) and l1.shape == l0.shape == (B,)
    assert float((x1 - x0).abs().max()) < Z_ATOL and torch.equal(x1, x2)
    # one BatchNorm in train(): not the engine's call
    m.WNs[3].F.pred.start[1].train()
    with torch.no_grad():
        m.reverse(z, h)
    assert stats()[0] == c0 + 2


# ---- the shipped architecture once -------------------------------------------------------------------------------------------------
def test_shipped_architecture_round_trip_and_infer(graphs_off):
    arch = mgg.ARCH_FULL
    ref = np.load(os.path.join(GOLD, "model_mg_full.npz"))
    m = cm.MelGlow(memory_efficient=True, **arch)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(m, "mg_full/", arch).items()}
    at = {"running_mean": 0, "running_var": 0}
    for k in sd:                                   # the fixture keeps the post-step running statistics concatenated in buffer order
        kind = k.rsplit(".", 1)[-1]
        if kind in at:
            n = sd[k].numel()
            sd[k] = torch.from_numpy(ref[kind][at[kind]:at[kind] + n].copy())
            at[kind] += n
    assert at["running_mean"] == ref["running_mean"].size and at["running_var"] == ref["running_var"].size
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    frames, hop = 62, arch["hop_size"]
    audio, h = mgg.inputs("mge_full", 1, frames * hop, arch["n_mels"], hop)
    audio, h = torch.from_numpy(audio).to(DEV), torch.from_numpy(h).to(DEV)
    c0, l0 = stats()
    with torch.no_grad():
        z, ld = m(audio, h)
        x, ldr = m.reverse(z, h)
    assert stats() == (c0 + 2, l0 + 2 * arch["flows"] * arch["depth"])
    assert bool(torch.isfinite(z).all()) and float((x - audio).abs().max()) < 1e-4
    assert float((ld + ldr).abs().max()) < 1e-3 * max(1.0, float(ld.abs().max()))
    out = m.infer(h[0])
    assert out.shape == (frames * hop,) and bool(torch.isfinite(out).all())
    assert stats()[0] == c0 + 3
