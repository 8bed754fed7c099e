"""MRWaveGlow on the MI355X (-m gpu): the coupling blocks at the WN shapes only this model has, against the same block in plain float64
torch; the whole model against the reference's own training steps (tests/golden/mr/, made by make_golden_mrwaveglow.py); round trips,
sampling, run-to-run identity, the checkpoint path and the shipped size.  The plumbing kernels one by one:
test_gpu_mrwaveglow_kernels.py.

Bars (the project's): z and log_s 1e-4 abs, loss 1e-6 abs, logdet rtol 1e-4, every gradient within 1e-4 of its tensor's max-abs."""
import os

import numpy as np
import pytest
import torch

import fill
import make_golden_mrwaveglow as mrg
from oracle import torch_cpu
import constant_memory_waveglow_amd as cm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mr")
Z_ATOL, LOSS_ATOL, GRAD_RTOL = 1e-4, 1e-6, 1e-4
PRECISIONS = ["f32", "bf16x3", "bf16x3p"]
DEFAULT = "bf16x3p"


def set_precision(monkeypatch, precision):
    """the arithmetic of the contractions is read from WG_PRECISION when a block is built (include/wgflow.h WG_PREC_*)"""
    if precision == DEFAULT:
        monkeypatch.delenv("WG_PRECISION", raising=False)
    else:
        monkeypatch.setenv("WG_PRECISION", precision)


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def fan_in_one(name, p):
    """A start conv with one input channel under weight norm is w = g sign(v): the exact gradient w.r.t. v is zero, and what either side
    holds there is rounding noise.  It is held to 1e-6 (16 roundings) of the gradient of the g next to it -- the scale of the two terms
    that cancel -- on both sides, as the other models' tests hold WN2D's; a ratio to the tensor's own max says nothing."""
    return name.endswith("start.weight_v") and p[0].numel() == 1


def assert_noise(got, want_max, g_scale, what):
    got = float(torch.as_tensor(got).detach().abs().max())
    print("fan-in-1 weight_v", what, "ours %.3e reference %.3e scale %.3e" % (got, float(want_max), float(g_scale)))
    assert got < 1e-6 * float(g_scale) and float(want_max) < 1e-6 * float(g_scale), what


# ---- the couplings at MR's WN shapes ---------------------------------------------------------------------------------------------
# (in_channels, aux_channels): the shipped levels and prior, the super-resolution levels, n_group 16 with four levels
MR_SHAPES = [(2, 84), (1, 82), (1, 80), (2, 4), (1, 2), (4, 88)]
WN_KW = dict(dilation_channels=32, residual_channels=32, skip_channels=32, depth=2, radix=3, bias=False)
_BLOCK64 = {}


def block_case(ic, aux):
    """inputs, parameter values and seeds of one coupling case (numpy / CPU, the same for every mode)"""
    B, T = 2, 131
    tag = "mrblock/%d_%d/" % (ic, aux)
    probe = cm.AffineCouplingBlock(cm.WN, in_channels=ic, aux_channels=aux, **WN_KW)
    return dict(x=torch.from_numpy(fill.normal(tag + "x", (B, 2 * ic, T))), y=torch.from_numpy(fill.normal(tag + "y", (B, aux, T))),
                gz=torch.from_numpy(fill.normal(tag + "gz", (B, 2 * ic, T))), gl=torch.from_numpy(fill.normal(tag + "gl", (B, ic, T))),
                params={k: torch.from_numpy(np.asarray(v)) for k, v in mrg.param_values(probe, tag).items()})


def block64(ic, aux, reverse):
    """the same block as plain float64 torch on the CPU (oracle/torch_cpu.py's WN): computed once per case and direction"""
    key = (ic, aux, reverse)
    if key not in _BLOCK64:
        case = block_case(ic, aux)
        probe = cm.AffineCouplingBlock(cm.WN, in_channels=ic, aux_channels=aux, **WN_KW)
        probe.load_state_dict(case["params"])
        table = [t.detach().double().requires_grad_(True) for t in probe.F.param_table()]
        x, y = case["x"].double().requires_grad_(True), case["y"].double().requires_grad_(True)
        xa, xb = x[:, :ic], x[:, ic:]
        log_s, t = torch_cpu._wn_forward(table, xa, y, WN_KW["depth"], WN_KW["residual_channels"], WN_KW["radix"])
        if reverse:
            z, ret = torch.cat((xa, (xb - t) / log_s.exp()), 1), -log_s
        else:
            z, ret = torch.cat((xa, xb * log_s.exp() + t), 1), log_s
        grads = torch.autograd.grad((z * case["gz"].double()).sum() + (ret * case["gl"].double()).sum(), [x, y] + table)
        names = [n for n, _ in probe.F.named_parameters()]
        by_param = {id(p): g for p, g in zip(probe.F.param_table(), grads[2:])}
        _BLOCK64[key] = dict(z=z.detach(), log_s=ret.detach(), dx=grads[0], dy=grads[1],
                             grads={n: by_param[id(p)] for n, p in zip(names, probe.F.parameters())})
    return _BLOCK64[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("ic,aux", MR_SHAPES)
def test_coupling_at_mr_shapes_vs_float64(ic, aux, precision, monkeypatch):
    set_precision(monkeypatch, precision)
    case = block_case(ic, aux)
    for reverse in (False, True):
        want = block64(ic, aux, reverse)
        for memory_efficient in (True, False):
            what = (ic, aux, precision, reverse, memory_efficient)
            block = cm.AffineCouplingBlock(cm.WN, memory_efficient=memory_efficient, in_channels=ic, aux_channels=aux, **WN_KW)
            block.load_state_dict(case["params"])
            block = block.to(DEV)
            x = case["x"].to(DEV).requires_grad_(True)
            y = case["y"].to(DEV).requires_grad_(True)
            z, log_s = block.reverse(x, y) if reverse else block(x, y)
            assert (x.untyped_storage().size() == 0) == memory_efficient, what
            assert float((z.detach().cpu() - want["z"]).abs().max()) < Z_ATOL, what
            assert float((log_s.detach().cpu() - want["log_s"]).abs().max()) < Z_ATOL, what
            ((z * case["gz"].to(DEV)).sum() + (log_s * case["gl"].to(DEV)).sum()).backward()
            assert float((x.detach().cpu() - case["x"]).abs().max()) < 1e-5, what       # the freed input, rebuilt from the output
            assert rel(x.grad, want["dx"]) < GRAD_RTOL, what
            assert rel(y.grad, want["dy"]) < GRAD_RTOL, what
            for n, p in block.F.named_parameters():
                if fan_in_one(n, p):
                    assert_noise(p.grad, want["grads"][n].abs().max(), want["grads"][n[:-1] + "g"].abs().max(), (what, n))
                    continue
                assert rel(p.grad, want["grads"][n]) < GRAD_RTOL, (what, n)


# ---- the model against the reference's training step -----------------------------------------------------------------------------
def build(name, **over):
    arch, tag, me, rmode, sr = mrg.CASES.get(name, (mrg.ARCH_FULL, "mr_full/", True, False, False))
    kw = dict(memory_efficient=me, reverse_mode=rmode, super_resolution=sr)
    kw.update(over)
    m = cm.MRWaveGlow(**kw, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mrg.param_values(m, tag).items()})
    return m.to(DEV), arch


def data(shape_tag, arch):
    B, N, frames = mrg.SHAPES[shape_tag]
    return mrg.inputs(shape_tag, B, N, arch["n_mels"], frames)


def step(m, arch, shape_tag, h_grad=True):
    audio, h = data(shape_tag, arch)
    x = torch.from_numpy(audio).to(DEV)
    ht = torch.from_numpy(h).to(DEV).requires_grad_(h_grad)
    z, ld = m(x, ht)
    loss = cm.WaveGlowLoss(fill.SIGMA)(z, ld)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.from_numpy(audio)) and torch.equal(ht.detach().cpu(), torch.from_numpy(h))      # the caller's tensors
    return z, ld, loss, ht


SMALL = [(n, DEFAULT) for n in mrg.CASES] + [(n, p) for n in ("mr_small", "mr_ragged") for p in ("f32", "bf16x3")]


@pytest.mark.parametrize("name,precision", SMALL)
def test_small_model_vs_reference(name, precision, monkeypatch):
    set_precision(monkeypatch, precision)
    ref = mrg.load(name, GOLD)
    m, arch = build(name)
    z, ld, loss, ht = step(m, arch, mrg.INPUT_TAG[name])
    assert float((z.detach().cpu() - torch.from_numpy(ref["z"])).abs().max()) < Z_ATOL
    assert abs(float(loss) - float(ref["loss"])) < LOSS_ATOL
    np.testing.assert_allclose(ld.detach().cpu().numpy(), ref["logdet"], rtol=1e-4, atol=1e-7 * ref["z"].size)
    for n, p in m.named_parameters():
        if fan_in_one(n, p):
            assert_noise(p.grad, np.abs(ref["grad::" + n]).max(), np.abs(ref["grad::" + n[:-1] + "g"]).max(), n)
        else:
            assert rel(p.grad, ref["grad::" + n]) < GRAD_RTOL, n
    assert len(list(m.parameters())) == sum(k.startswith("grad::") for k in ref)
    assert rel(ht.grad, ref["dh"]) < GRAD_RTOL
    m.eval()
    with torch.no_grad():
        zc = z.detach().clone()
        xr, ldr = m.reverse(zc, ht.detach())
    assert torch.equal(zc, z.detach())
    assert float((xr.cpu() - torch.from_numpy(ref["x_inv_eval"])).abs().max()) < Z_ATOL
    np.testing.assert_allclose(ldr.cpu().numpy(), ref["logdet_inv_eval"], rtol=1e-4, atol=1e-7 * ref["z"].size)


# ---- properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mr_small", "mr_small_nme", "mr_small_rm", "mr_small_sr", "mr_ragged"])
def test_round_trip_infer_and_determinism(name):
    m, arch = build(name)
    m.eval()
    audio, h = data(mrg.INPUT_TAG[name], arch)
    x, ht = torch.from_numpy(audio).to(DEV), torch.from_numpy(h).to(DEV)
    with torch.no_grad():
        z, ld = m(x, ht)
        xr, ldr = m.reverse(z.clone(), ht)
    assert float((xr - x).abs().max()) < 1e-4
    assert float((ld + ldr).abs().max()) <= 1e-4 * float(ld.abs().max())
    assert torch.equal(x.cpu(), torch.from_numpy(audio)) and torch.equal(ht.cpu(), torch.from_numpy(h))
    B, frames = ht.size(0), ht.size(2)
    out = m.infer(ht, sigma=0.6)
    assert out.shape == (B, frames * arch["hop_size"]) and bool(torch.isfinite(out).all())
    assert m.infer(ht[0]).shape == (frames * arch["hop_size"],)

    m.train()
    runs = []
    for _ in range(2):
        m2, _ = build(name)
        z, ld, loss, ht2 = step(m2, arch, mrg.INPUT_TAG[name])
        runs.append([z.detach().cpu(), ld.detach().cpu(), loss.detach().cpu(), ht2.grad.cpu()] + [p.grad.cpu() for p in m2.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_checkpoint_in_the_reference_layout_and_weight_norm_removal(tmp_path):
    """The parameter names the reference's own step recorded (the fixture's gradient keys) are a state dict this module loads with
    strict=True, through a file; folding the weight norms away (utils.remove_weight_norms, as inference does) leaves infer unchanged."""
    ref = mrg.load("mr_small", GOLD)
    names = [k.split("::", 1)[1] for k in ref if k.startswith("grad::")]
    m, arch = build("mr_small")
    values = mrg.param_values(m, "mr_small/")
    assert sorted(names) == sorted(values)
    path = os.path.join(str(tmp_path), "checkpoint.pt")
    torch.save({n: torch.from_numpy(np.asarray(values[n])) for n in names}, path)
    fresh = cm.MRWaveGlow(memory_efficient=True, **arch)
    result = fresh.load_state_dict(torch.load(path), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    fresh = fresh.to(DEV).eval()
    _, h = data("mr_small", arch)
    ht = torch.from_numpy(h).to(DEV)
    torch.manual_seed(7)
    before = fresh.infer(ht, sigma=0.6)
    torch.manual_seed(7)
    assert torch.equal(m.eval().infer(ht, sigma=0.6), before)          # the same weights, loaded the other way
    fresh.apply(cm.remove_weight_norms)
    assert not any(k.endswith("weight_g") for k in fresh.state_dict())
    torch.manual_seed(7)
    after = fresh.infer(ht, sigma=0.6)
    assert float((after - before).abs().max()) < 1e-5


def test_shipped_config_vs_reference_summary():
    ref = np.load(os.path.join(GOLD, "model_mr_full.npz"))
    m, arch = build("mr_full")
    assert len(m.state_dict()) == 456 and sum(p.numel() for p in m.parameters()) == 53_735_520
    z, ld, loss, _ = step(m, arch, "mr_full", h_grad=False)
    zz = z.detach().cpu().numpy()
    assert np.abs(zz[:, :256] - ref["z_head"]).max() < Z_ATOL and np.abs(zz[:, -256:] - ref["z_tail"]).max() < Z_ATOL
    np.testing.assert_allclose(np.sqrt((zz.astype(np.float64) ** 2).sum(1)), ref["z_item_norm"], rtol=1e-5)
    assert abs(float(loss) - float(ref["loss"])) < LOSS_ATOL
    np.testing.assert_allclose(ld.detach().cpu().numpy(), ref["logdet"], rtol=1e-4)
    for i, (n, p) in enumerate(m.named_parameters()):
        g = p.grad.detach().double().cpu().numpy().ravel()
        scale = float(ref["grad_max"][i])
        if fan_in_one(n, p):                                          # (weight_g is the parameter just before weight_v)
            assert_noise(p.grad, scale, ref["grad_max"][i - 1], n)
            continue
        assert abs(np.abs(g).max() - scale) <= GRAD_RTOL * scale + 1e-30, n
        assert abs(np.sqrt((g ** 2).sum()) - float(ref["grad_norm"][i])) <= 1e-4 * float(ref["grad_norm"][i]) + 1e-30, n
        assert np.abs(g[:8] - ref["grad_head"][i][:min(8, g.size)]).max() <= GRAD_RTOL * scale + 1e-30, n
