"""WaveFlow on the MI355X (-m gpu) at every height wf_check admits and past one 256-column block.  The WaveFlow cases of
test_gpu_parity.py run at n_group 8 x 96 columns, 64 x 24 and the shipped 64 x 250; here (fill.WF_CONFIGS / fill.WF_SHAPES, T = columns):

    wf16       n_group 16, T 40    upsampler at stride 16 with 33 taps
    wf32       n_group 32, T 33    height dilations 1,2,4,1,2,4,1,2; stride 8, 17 taps; T = the last column the upsampler produces
    wf128      n_group 128, T 13   height dilations 1 .. 64, 1; stride 2, 5 taps; T at the upsampler's maximum
    wf8_long   n_group 8, T 321    two blocks of 256 columns in every one-thread-per-column kernel and in wf_couple_row_kernel's t0 loop
                                   (a partial second pass), six 64-column tiles per item = 18 Gram partials, T at the maximum, F + 1 = 10
    wf64_long  n_group 64, T 259   259 = 256 + 3 = 4 * 64 + 3: five Gram partials (an odd count for the two-at-a-time sum), a column tail
                                   behind four full tiles in wf_rowsum_s_kernel, F + 1 = 66 padded frames walked eight at a time
    wf8_wide   65 items, T 8       the second block of wf_logdet_kernel (blocks of 64 items); F = 1: every clamp of the upsampler's
                                   backward lands on frame 0

with the flip (every case), use_conv1x1=True (suffix c: wf_hmix / wf_hgram / wf_hgram_reduce / lu_big_kernel; wf128c needs 66 560 B of
LDS for lu_big_kernel and for wf_hgram_kernel, the only opt-in above 48 KB on this path) and WN2D(bias=True) at 128 rows (wf128b: the
ones segment next to a height dilation of 64).

Expected values: the reference's own run (tests/golden/wf/model_<name>.npz, make_golden_waveflow.py) AND a float64 oracle run, which
gives every gradient in full where the fixture keeps norm / head / max -- oracle/torch_cpu.py for the flip, oracle/wf_oracle.c for the
1x1 and bias variants, both pinned to these fixtures by tests/test_oracle_golden.py.  wf64_longc is held to its fixture alone (the C
oracle takes about 30 s there); wf8_wide to the oracle alone (with the 1x1 its logdets are near zero and the reference's own fp32
logdet sits outside logdet_close of float64, so it is flip-only and has no fixture).

Bars: those of test_gpu_parity.py, unchanged -- z / x 1e-4, logdet rtol 1e-4 + 1e-7 per sample, loss 1e-6, every gradient within 1e-4
of its tensor's max, the upsampled conditioning 2e-6.

The library's launch-site record (wg_timer_read_name) names the launches of the timed kernel classes only -- the conv, weight-gradient,
layer and thin kernels; none of WaveFlow's own kernels is in a class, so there is no name of wf_couple_row_kernel to assert on.  That
kernel is the only route a mode-2 coupling can take (Cs % 32 == 0, csrc/wgflow.hip wf_couple): the inverse checks below are its check."""
import os

import numpy as np
import pytest
import torch

import fill
import constant_memory_waveglow_amd as cm

pytestmark = pytest.mark.gpu

Z_ATOL, LOSS_ATOL, GRAD_RTOL = 1e-4, 1e-6, 1e-4
PRECISIONS = ["f32", "bf16x3", "bf16x3p"]


@pytest.fixture(params=PRECISIONS, autouse=True)
def precision(request, monkeypatch):
    """The three arithmetic modes of the contraction kernels (include/wgflow.h WG_PREC_*), as in test_gpu_parity.py: same bars for all."""
    monkeypatch.setenv("WG_PRECISION", request.param)
    return request.param


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu suite needs the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


def relmax(a, b):
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


def logdet_close(a, b, N):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-7 * N))


CASES = fill.WF_SHAPE_FIXTURES + ["wf8_wide"]
NO_ORACLE = {"wf64_longc"}
_ORACLE = {}


def case_inputs(name):
    cfg = fill.WF_CONFIGS[name]
    B, N, F = fill.WF_SHAPES[name]
    specs = fill.waveflow_param_specs(cfg)
    P = fill.fill_params(specs, name + "/")
    audio, mel = fill.waveflow_inputs(name, B, N, F, cfg["n_mels"])
    return cfg, specs, P, audio, mel


def oracle_once(name):
    """The float64 oracle's training step of a case: it does not depend on the GPU's arithmetic mode, so it runs for the first of the
    three modes and is dropped when the third has taken it."""
    if name in NO_ORACLE:
        return None
    if name not in _ORACLE:
        cfg, specs, P, audio, mel = case_inputs(name)
        tab = fill.table(specs, P)
        if cfg.get("use_conv1x1") or cfg.get("bias"):
            from oracle import wf_oracle as wfo
            r = wfo.train_step(wfo.make_config(**cfg), tab, audio, mel, fill.SIGMA, need_dmel=True, double=True)
        else:
            from oracle import torch_cpu
            _, quota, firsts = torch_cpu.host_cpu_budget()
            cores = max(1, int(quota) if quota else len(firsts))
            workers = max(1, min(audio.shape[0], cores // 2, torch_cpu.MAX_WORKERS))
            r = torch_cpu.train_step_parallel(dict(cfg, model="waveflow"), tab, audio, mel, fill.SIGMA, workers=workers,
                                              threads=max(1, min(8, cores // workers)), need_dh=True, double=True)
            r["dmel"] = r["dh"]
        _ORACLE[name] = [r, 0]
    entry = _ORACLE[name]
    entry[1] += 1
    if entry[1] == len(PRECISIONS):
        del _ORACLE[name]
    return entry[0]


def fixture_of(golden_dir, name):
    return np.load(os.path.join(golden_dir, "wf", "model_%s.npz" % name)) if name in fill.WF_SHAPE_FIXTURES else None


def build(name, dev):
    cfg, specs, P, audio, mel = case_inputs(name)
    m = cm.WaveFlow(memory_efficient=False, **dict({"use_conv1x1": False, "bias": False}, **cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return m.to(dev), cfg, specs, audio, mel


def step(m, audio, mel, dev):
    ht = T(mel, dev).requires_grad_(True)
    z, logdet = m(T(audio, dev), ht)
    loss = cm.WaveGlowLoss(fill.SIGMA)(z, logdet)
    loss.backward()
    return z, logdet, loss, ht


@pytest.mark.parametrize("name", CASES)
def test_waveflow_shape_step_and_inverse(dev, golden_dir, precision, name):
    """Forward + NLL + backward (mel.requires_grad) and the row-by-row inverse of one case against the reference's run and the float64
    oracle: every element of z, logdet, d loss / d mel and of every gradient; the inverse from the reference's z."""
    gold, ref = fixture_of(golden_dir, name), oracle_once(name)
    assert gold is not None or ref is not None
    m, cfg, specs, audio, mel = build(name, dev)
    B, N = audio.shape
    assert bool(cfg.get("use_conv1x1")) == hasattr(m, "invconv1x1")
    z, logdet, loss, ht = step(m, audio, mel, dev)
    named = dict(m.named_parameters())
    assert sorted(named) == sorted(n for n, _, _ in specs)
    worst = 0.0
    for tag, want in (("oracle", ref), ("fixture", gold)):
        if want is None:
            continue
        print("%s [%s] vs %s: |dz| %.2e  |dlogdet| %.2e  |dloss| %.2e  dmel %.2e of max" % (
            name, precision, tag, float(np.abs(npy(z) - want["z"]).max()), float(np.abs(npy(logdet) - want["logdet"]).max()),
            abs(float(loss) - float(want["loss"])), relmax(npy(ht.grad), want["dmel"])))
        assert np.abs(npy(z) - want["z"]).max() < Z_ATOL, tag
        assert logdet_close(npy(logdet), want["logdet"], N), tag            # (every item: 65 of them in wf8_wide)
        assert abs(float(loss) - float(want["loss"])) < LOSS_ATOL, tag
        assert relmax(npy(ht.grad), want["dmel"]) < GRAD_RTOL, tag
    for i, (n, _, _) in enumerate(specs):
        g = npy(named[n].grad)
        assert np.isfinite(g).all(), n
        if n.endswith("start.weight_v"):
            # Conv2d(1, C, 1) under weight norm: the exact gradient w.r.t. v is zero (w = g * sign(v)); rounding noise on every side
            assert np.abs(g).max() < 1e-5 * np.abs(npy(named[n[:-1] + "g"].grad)).max(), n
            continue
        if ref is not None:
            e = relmax(g, ref["grads"][i])
            worst = max(worst, e)
            assert e < GRAD_RTOL, n
        if gold is not None:
            nh = min(g.size, gold["grad_head"].shape[1])
            assert np.abs(g.ravel()[:nh] - gold["grad_head"][i][:nh]).max() / max(float(gold["grad_max"][i]), 1e-30) < GRAD_RTOL, n
            if "grad::" + n in gold:
                assert relmax(g, gold["grad::" + n]) < GRAD_RTOL, n
            if ref is None:
                # no oracle run to hold every element to: the norm of the whole tensor, as for the summary fixtures of the timed workloads
                gn = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
                assert abs(gn - float(gold["grad_norm"][i])) <= 1e-4 * float(gold["grad_norm"][i]) + 1e-12, n
    print("%s [%s]: worst gradient vs oracle %.2e of its tensor's max" % (name, precision, worst))
    z_in = gold["z"] if gold is not None else ref["z"].astype(np.float32)
    with torch.no_grad():
        x, ld = m.reverse(T(z_in, dev), ht.detach())
    print("%s [%s] inverse: |x - audio| %.2e" % (name, precision, float(np.abs(npy(x) - audio).max())))
    assert np.abs(npy(x) - audio).max() < Z_ATOL
    if gold is not None:
        assert np.abs(npy(x) - gold["x_inv"]).max() < Z_ATOL
        assert logdet_close(npy(ld), gold["logdet_inv"], N)
        with torch.no_grad():
            y_up = npy(m._upsample_h(ht.detach()))
        assert y_up.shape == gold["y_up"].shape and np.abs(y_up - gold["y_up"]).max() < 2e-6
    if ref is not None:
        assert logdet_close(-npy(ld), ref["logdet"], N)


def test_wf128c_takes_the_lds_opt_in(dev, golden_dir, precision):
    """use_conv1x1 at 128 rows: lu_big_kernel (packing) needs (128 * 129 + 128) floats and wf_hgram_kernel (backward) 2 * 128 * 65 floats
    of dynamic LDS, 66 560 B each, above the 48 KB a kernel gets without asking -- the one place on the WaveFlow path where
    ensure_dynamic_lds has to ask (csrc/wgflow.hip wf_check documents the case as supported).  It must build, pack, step and invert
    without an error code, and what the two kernels produce must be right: logdet carries T * logdet W of both matrices, the inverse
    applies both W^-1, and the two invconv1x1 gradients are the Gram sums."""
    name = "wf128c"
    H = fill.WF_CONFIGS[name]["n_group"]
    assert (H * (H + 1) + H) * 4 == 66560 and 2 * H * 65 * 4 == 66560 and 66560 > 48 * 1024
    gold = fixture_of(golden_dir, name)
    m, cfg, specs, audio, mel = build(name, dev)
    N = audio.shape[1]
    z, logdet, loss, ht = step(m, audio, mel, dev)           # (a refused opt-in or a failed launch raises WgError here)
    torch.cuda.synchronize()
    assert logdet_close(npy(logdet), gold["logdet"], N)
    assert np.abs(npy(z) - gold["z"]).max() < Z_ATOL
    mix = [n for n, _, _ in specs if "invconv1x1" in n]
    assert len(mix) == 2
    for n in mix:
        g = npy(dict(m.named_parameters())[n].grad)
        assert g.shape == (H, H, 1) and relmax(g, gold["grad::" + n]) < GRAD_RTOL, n
    with torch.no_grad():
        x, ld = m.reverse(T(gold["z"], dev), ht.detach())
    assert np.abs(npy(x) - audio).max() < Z_ATOL and logdet_close(npy(ld), gold["logdet_inv"], N)


@pytest.mark.parametrize("name", ["wf8_long", "wf64_long"])
def test_batch_items_are_independent_past_the_block_edges(dev, precision, name):
    """z of item 0 run alone equals z[0] of a batch, at widths where an item spans two column blocks.  wf8_long is a batch of three;
    wf64_long's fixture is one item, so its batch here is two items of the same width (fill.py draws the rows of a batch one after the
    other: item 0 of the two is the fixture's item)."""
    m, cfg, specs, audio, mel = build(name, dev)
    B, N, F = fill.WF_SHAPES[name]
    if B == 1:
        a2, m2 = fill.waveflow_inputs(name, 2, N, F, cfg["n_mels"])
        assert np.array_equal(a2[:1], audio) and np.array_equal(m2[:1], mel)
        audio, mel = a2, m2
    with torch.no_grad():
        z, ld = m(T(audio, dev), T(mel, dev))
        z1, ld1 = m(T(audio[:1], dev), T(mel[:1], dev))
    assert z.shape == (audio.shape[0], N) and z1.shape == (1, N)
    assert float((z1 - z[:1]).abs().max()) < 1e-5
    assert logdet_close(npy(ld1), npy(ld[:1]), N)
