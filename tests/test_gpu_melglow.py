"""MelGlow on the MI355X (-m gpu): the LVC layer and the predictor against the float64 restatements of golden/mg_ref64.py (the kernels
one by one at ragged shapes: test_gpu_melglow_kernels.py), the whole model against
the reference's own training steps (tests/golden/mg/, made by make_golden_melglow.py), round trips, sampling and run-to-run identity.

Bars: z 1e-4 abs, loss 1e-6 abs, logdet rtol 1e-4, every gradient within 1e-4 of its tensor's max-abs, BatchNorm running statistics
1e-5 relative, num_batches_tracked exact."""
import os

import numpy as np
import pytest
import torch

import fill
import make_golden_melglow as mgg
from mg_ref64 import layer64, predictor64, wnorm64
import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import melglow as mg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mg")
Z_ATOL, LOSS_ATOL, GRAD_RTOL, STAT_RTOL = 1e-4, 1e-6, 1e-4, 1e-5


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


# ---- the LVC layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nf,L,dilation,last", [(2, 5, 32, 64, False), (2, 5, 32, 64, True), (1, 1, 32, 4, False), (3, 4, 16, 1, False),
                                                   (2, 6, 32, 8, True)])
def test_lvc_layer_vs_float64(B, nf, L, dilation, last):
    R = D = S = 16
    layer = mg.NonCausalLayerLVC(dilation, D, R, S, 3, False, last_layer=last)
    layer.apply(cm.add_weight_norms)
    layer = layer.to(DEV)
    T = nf * L
    x = torch.from_numpy(fill.normal("lvc/x%d" % dilation, (B, R, T))).to(DEV).requires_grad_(True)
    w = torch.from_numpy(fill.normal("lvc/w%d" % dilation, (B, nf, 2 * D, R, 3), 0.15)).to(DEV).requires_grad_(True)
    res, skip = layer(x, w)
    g_skip = torch.from_numpy(fill.normal("lvc/gs", tuple(skip.shape))).to(DEV)
    loss = (skip * g_skip).sum()
    if not last:
        g_res = torch.from_numpy(fill.normal("lvc/gr", tuple(res.shape))).to(DEV)
        loss = loss + (res * g_res).sum()
    loss.backward()

    x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    g64, v64 = (layer.W_o.weight_g.detach().double().requires_grad_(True), layer.W_o.weight_v.detach().double().requires_grad_(True))
    r64, s64 = layer64(x64, w64, dilation, wnorm64(g64, v64), R, last)
    l64 = (s64 * g_skip.double()).sum() + (0 if last else (r64 * g_res.double()).sum())
    l64.backward()
    assert rel(skip, s64) < 1e-5
    if not last:
        assert rel(res, r64) < 1e-5
    assert rel(x.grad, x64.grad) < GRAD_RTOL
    assert rel(w.grad, w64.grad) < GRAD_RTOL
    assert rel(layer.W_o.weight_g.grad, g64.grad) < GRAD_RTOL
    assert rel(layer.W_o.weight_v.grad, v64.grad) < GRAD_RTOL


# ---- the predictor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_predictor_vs_float64(training):
    pred = mg.Predictor(80, 96, 16, 2, False, 7)
    vals = {k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(pred, "pred/", dict(residual_channels=8, radix=3)).items()}
    pred.load_state_dict(vals)
    pred = pred.to(DEV).train(training)
    y = torch.from_numpy(fill.normal("pred/y", (3, 80, 11))).to(DEV).requires_grad_(True)
    out = pred(y)
    gout = torch.from_numpy(fill.normal("pred/g", tuple(out.shape))).to(DEV)
    (out * gout).sum().backward()

    ref = mg.Predictor(80, 96, 16, 2, False, 7)
    ref.load_state_dict(vals)
    ref = ref.double().to(DEV)
    y64 = y.detach().double().requires_grad_(True)
    o64, bufs = predictor64(ref, y64, training)
    (o64 * gout.double()).sum().backward()
    assert out.shape == o64.shape == (3, 7 * 96, 11)
    assert rel(out, o64) < 1e-5
    assert rel(y.grad, y64.grad) < GRAD_RTOL
    for (n, p), p64 in zip(pred.named_parameters(), ref.parameters()):
        assert rel(p.grad, p64.grad) < GRAD_RTOL, n
    for m, m64 in zip(pred.modules(), ref.modules()):
        if isinstance(m, torch.nn.BatchNorm1d):
            rm, rv = bufs[id(m64)]
            assert rel(m.running_mean, rm) < STAT_RTOL and rel(m.running_var, rv) < STAT_RTOL
            assert int(m.num_batches_tracked) == 3 + int(training)


# ---- the model against the reference's training step -----------------------------------------------------------------------------
def build(name, memory_efficient=None, reverse_mode=None):
    arch, tag, me, rmode = mgg.CASES.get(name, (mgg.ARCH_FULL, "mg_full/", True, False))
    m = cm.MelGlow(memory_efficient=me if memory_efficient is None else memory_efficient,
                   reverse_mode=rmode if reverse_mode is None else reverse_mode, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(m, tag, arch).items()})
    return m.to(DEV), arch


def step(m, arch, shape_tag, h_grad=True):
    B, N = mgg.SHAPES[shape_tag]
    audio, h = mgg.inputs(shape_tag, B, N, arch["n_mels"], arch["hop_size"])
    x = torch.from_numpy(audio).to(DEV)
    ht = torch.from_numpy(h).to(DEV).requires_grad_(h_grad)
    z, ld = m(x, ht)
    loss = cm.WaveGlowLoss(fill.SIGMA)(z, ld)
    loss.backward()
    torch.cuda.synchronize()
    return z, ld, loss, ht


@pytest.mark.parametrize("name", ["mg_small", "mg_small_nme", "mg_small_rm", "mg_ragged"])
def test_small_model_vs_reference(name):
    ref = np.load(os.path.join(GOLD, "model_%s.npz" % name))
    m, arch = build(name)
    z, ld, loss, ht = step(m, arch, mgg.INPUT_TAG[name])
    assert float((z.detach().cpu() - torch.from_numpy(ref["z"])).abs().max()) < Z_ATOL
    assert abs(float(loss) - float(ref["loss"])) < LOSS_ATOL
    np.testing.assert_allclose(ld.detach().cpu().numpy(), ref["logdet"], rtol=1e-4, atol=1e-7 * ref["z"].size)
    for n, p in m.named_parameters():
        assert rel(p.grad, ref["grad::" + n]) < GRAD_RTOL, n
    assert rel(ht.grad, ref["dh"]) < GRAD_RTOL
    per_step = 2 if mgg.CASES[name][2] else 1
    for n, b in m.named_buffers():
        want = ref["buf::" + n]
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(want) == 3 + per_step, n
        else:
            assert rel(b, want) < STAT_RTOL, n
    m.eval()
    with torch.no_grad():
        xr, ldr = m.reverse(z.detach().clone(), ht.detach())
    assert float((xr.cpu() - torch.from_numpy(ref["x_inv_eval"])).abs().max()) < Z_ATOL
    np.testing.assert_allclose(ldr.cpu().numpy(), ref["logdet_inv_eval"], rtol=1e-4, atol=1e-7 * ref["z"].size)


def test_shipped_config_vs_reference_summary():
    ref = np.load(os.path.join(GOLD, "model_mg_full.npz"))
    m, arch = build("mg_full")
    assert len(m.state_dict()) == 732 and sum(p.numel() for p in m.parameters()) == 77_260_688
    z, ld, loss, _ = step(m, arch, "mg_full", h_grad=False)
    zz = z.detach().cpu().numpy()
    assert np.abs(zz[:, :256] - ref["z_head"]).max() < Z_ATOL and np.abs(zz[:, -256:] - ref["z_tail"]).max() < Z_ATOL
    np.testing.assert_allclose(np.sqrt((zz.astype(np.float64) ** 2).sum(1)), ref["z_item_norm"], rtol=1e-5)
    assert abs(float(loss) - float(ref["loss"])) < LOSS_ATOL
    np.testing.assert_allclose(ld.detach().cpu().numpy(), ref["logdet"], rtol=1e-4)
    for i, (n, p) in enumerate(m.named_parameters()):
        g = p.grad.detach().double().cpu().numpy().ravel()
        scale = float(ref["grad_max"][i])
        assert abs(np.abs(g).max() - scale) <= GRAD_RTOL * scale + 1e-30, n
        assert abs(np.sqrt((g ** 2).sum()) - float(ref["grad_norm"][i])) <= 1e-4 * float(ref["grad_norm"][i]) + 1e-30, n
        assert np.abs(g[:8] - ref["grad_head"][i][:min(8, g.size)]).max() <= GRAD_RTOL * scale + 1e-30, n
    rm = np.concatenate([b.cpu().numpy().ravel() for n, b in m.named_buffers() if n.endswith("running_mean")])
    rv = np.concatenate([b.cpu().numpy().ravel() for n, b in m.named_buffers() if n.endswith("running_var")])
    assert np.abs(rm - ref["running_mean"]).max() <= STAT_RTOL * np.abs(ref["running_mean"]).max()
    assert np.abs(rv - ref["running_var"]).max() <= STAT_RTOL * np.abs(ref["running_var"]).max()
    for n, b in m.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(ref["buf::" + n]) == 5, n


# ---- properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory_efficient", [True, False])
def test_round_trip_infer_and_determinism(memory_efficient):
    round_trip_infer_and_determinism("mg_small", memory_efficient)


@pytest.mark.parametrize("memory_efficient", [True, False])
def test_ragged_round_trip_infer_and_determinism(memory_efficient):
    round_trip_infer_and_determinism("mg_ragged", memory_efficient)


def round_trip_infer_and_determinism(name, memory_efficient):
    m, arch = build(name, memory_efficient=memory_efficient)
    m.eval()
    B, N = mgg.SHAPES[name]
    audio, h = mgg.inputs(name, B, N, arch["n_mels"], arch["hop_size"])
    ht = torch.from_numpy(h).to(DEV)
    with torch.no_grad():
        z, ld = m(torch.from_numpy(audio).to(DEV), ht)
        xr, ldr = m.reverse(z.clone(), ht)
    assert float((xr.cpu() - torch.from_numpy(audio)).abs().max()) < 1e-4
    assert float((ld + ldr).abs().max()) < 1e-3
    audio_out = m.infer(ht, sigma=0.6)
    assert audio_out.shape == (B, ht.size(2) * arch["hop_size"]) and bool(torch.isfinite(audio_out).all())
    assert m.infer(ht[0]).shape == (ht.size(2) * arch["hop_size"],)

    m.train()
    runs = []
    for _ in range(2):
        m2, _ = build(name, memory_efficient=memory_efficient)
        z, ld, loss, ht2 = step(m2, arch, name)
        runs.append([z.detach().cpu(), ld.detach().cpu(), ht2.grad.cpu()] + [p.grad.cpu() for p in m2.parameters()] +
                    [b.cpu() for b in m2.buffers()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_wn_lvc_state_and_train_eval_switch():
    """WN_LVC on its own: eval() freezes the running statistics and uses them; train() moves them once per call."""
    arch = mgg.ARCH_SMALL
    kw = dict(in_channels=4, aux_channels=80, depth=arch["depth"], dilation_channels=16, residual_channels=16, skip_channels=16,
              predict_channels=8, predict_layers=1, radix=3, bias=False)
    wn = cm.WN_LVC(**kw)
    assert not hasattr(wn, "hip_dims")
    wn = wn.to(DEV)
    x = torch.from_numpy(fill.normal("wn/x", (2, 4, 8 * 32))).to(DEV)
    y = torch.from_numpy(fill.normal("wn/y", (2, 80, 8))).to(DEV)
    wn.eval()
    before = [b.clone() for b in wn.buffers()]
    with torch.no_grad():
        a = wn(x, y)
        b = wn(x, y)
    assert all(torch.equal(u, v) for u, v in zip(before, wn.buffers()))
    assert torch.equal(a[1], b[1])
    wn.train()
    with torch.no_grad():
        wn(x, y)
    assert int(wn.pred.start[1].num_batches_tracked) == 1
    assert not torch.equal(wn.pred.start[1].running_mean, before[0])
