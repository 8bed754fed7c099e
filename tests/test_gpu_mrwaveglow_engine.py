"""MRWaveGlow's one-call eval passes on the MI355X (-m gpu): wg_mr_forward / wg_mr_inverse behind MRWaveGlow.forward / reverse / infer in
eval() under no_grad, against the reference's own fixtures (tests/golden/mr/), against the module path of the same model at ragged
shapes and edge configurations, the plane kernels on their own against the float64 restatements of golden/mr_ref64.py, run-to-run and
graph-replay identity, and the calls that must stay on the module path.

Bars (those of test_gpu_mrwaveglow.py): x / z 1e-4 abs, logdet rtol 1e-4 with atol 1e-7 per sample.

The plane kernels: the Haar split and merge are single roundings of exact operands (a multiplication by 1/2 is exact), so they are held
bit for bit to float64 rounded to fp32.  The upsampling is an fma chain of two terms whose weights are themselves rounded (s = 5), so
float64 rounded once is not what any fp32 kernel gives: it is held bit for bit to wg_mr_upsample, the kernel whose arithmetic it
repeats, and to float64 within the project's fma-chain bound (n + 3) 2^-24 sum |a_i b_i|, as test_gpu_mrwaveglow_kernels.py holds that
kernel.

Engine against module path, measured on one MI355X over every case, every one of the six column counts, both directions and all three
arithmetic modes of test_engine_vs_module_path, and at the shipped architecture (DESIGN.md 11.1 has the figures): x and z bit-equal in
all three arithmetic modes (the engine runs the module path's kernels on the same values;
the planes' layout does not change a route), so bit equality is what the test holds; logdet differs by at most 6.0e-6 relative
(5.7e-5 with levels = 1, whose logdets are the smallest): the engine adds log_s per 64-column tile and then the tiles, torch adds the [B, c/2, T] tensor."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fill
import make_golden_mrwaveglow as mrg
import mr_ref64 as r64
import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import _lib, engine
from constant_memory_waveglow_amd._lib import check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mr")
Z_ATOL = 1e-4
NAN = float("nan")
PRECISIONS = ["f32", "bf16x3", "bf16x3p"]
DEFAULT = "bf16x3p"


def set_precision(monkeypatch, precision):
    if precision == DEFAULT:
        monkeypatch.delenv("WG_PRECISION", raising=False)
    else:
        monkeypatch.setenv("WG_PRECISION", precision)


def passes():
    return _lib.lib().wg_stat_mr_pass_calls()


@pytest.fixture
def engine_on(monkeypatch):
    monkeypatch.setenv("WG_GRAPHS", "0")
    monkeypatch.delenv("WG_MR_ENGINE", raising=False)


def check_logdet(got, want, size):
    np.testing.assert_allclose(got.cpu().numpy(), torch.as_tensor(want).cpu().numpy(), rtol=1e-4, atol=1e-7 * size)


def build(arch, tag, **kw):
    m = cm.MRWaveGlow(**kw, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mrg.param_values(m, tag).items()})
    return m.to(DEV).eval()


def fixture_model(name):
    arch, tag, me, rmode, sr = mrg.CASES[name]
    return build(arch, tag, memory_efficient=me, reverse_mode=rmode, super_resolution=sr), arch


def both_paths(m, fn, monkeypatch):
    """fn() under no_grad through the engine and through the module path of the same model; the counters say which one ran"""
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("WG_MR_ENGINE", flag)
        p0 = passes()
        with torch.no_grad():
            out[flag] = fn()
        assert passes() - p0 == (len(out[flag]) // 2 if flag == "1" else 0), flag
    monkeypatch.delenv("WG_MR_ENGINE")
    return out["1"], out["0"]


# ---- 1. the reference's fixtures -------------------------------------------------------------------------------------------------
GOLDEN = [(n, DEFAULT) for n in ("mr_small", "mr_small_nme", "mr_small_rm", "mr_small_sr")] + [("mr_ragged", p) for p in PRECISIONS]


@pytest.mark.parametrize("name,precision", GOLDEN)
def test_engine_vs_reference_fixture(name, precision, monkeypatch, engine_on):
    set_precision(monkeypatch, precision)
    ref = mrg.load(name, GOLD)
    m, arch = fixture_model(name)
    B, N, frames = mrg.SHAPES[mrg.INPUT_TAG[name]]
    audio, h = mrg.inputs(mrg.INPUT_TAG[name], B, N, arch["n_mels"], frames)
    x, ht, zref = torch.from_numpy(audio).to(DEV), torch.from_numpy(h).to(DEV), torch.from_numpy(ref["z"]).to(DEV)
    keep = (x.clone(), ht.clone(), zref.clone())
    with torch.no_grad():
        assert m._engine_route(x, ht)[0] is None and m._engine_route(zref, ht)[0] is None
        p0 = passes()
        z, ld = m(x, ht)
        xr, ldr = m.reverse(zref, ht)
        assert passes() - p0 == 2
    assert torch.equal(x, keep[0]) and torch.equal(ht, keep[1]) and torch.equal(zref, keep[2])       # the caller's tensors are only read
    dz, dx = float((z - zref).abs().max()), float((xr.cpu() - torch.from_numpy(ref["x_inv_eval"])).abs().max())
    print("%s %s: engine vs reference: max |dz| %.3e, max |dx| %.3e" % (name, precision, dz, dx))
    assert dz < Z_ATOL and dx < Z_ATOL
    check_logdet(ld, ref["logdet"], ref["z"].size)
    check_logdet(ldr, ref["logdet_inv_eval"], ref["z"].size)
    # WG_MR_ENGINE=0: the same calls never reach the passes
    monkeypatch.setenv("WG_MR_ENGINE", "0")
    with torch.no_grad():
        assert m._engine_route(x, ht)[0] == "WG_MR_ENGINE=0"
        p0 = passes()
        z0, _ = m(x, ht)
        assert passes() == p0
    assert float((z0 - zref).abs().max()) < Z_ATOL


# ---- 2. engine against the module path of the same model -------------------------------------------------------------------------
SMALL2 = dict(mrg.ARCH_SMALL, depth=2)
COLUMNS = [1, 7, 8, 13, 257, 260]          # 8 and 260 reach the 16-byte paths, the others the scalar tails; 257 and 260 pass one 256-thread block
# name -> (arch, parameter tag, constructor switches, batch); the fixtures' own architectures where they differ in kind, depth 2 otherwise
VS_MODULE = {
    "small_b1": (SMALL2, "mre/", dict(), 1), "small_b2": (SMALL2, "mre/", dict(), 2),
    "rm_b1": (SMALL2, "mre/", dict(reverse_mode=True), 1), "rm_b2": (SMALL2, "mre/", dict(reverse_mode=True), 2),
    "sr_b1": (SMALL2, "mre_sr/", dict(super_resolution=True), 1), "sr_b2": (SMALL2, "mre_sr/", dict(super_resolution=True), 2),
    "ragged": (mrg.ARCH_RAGGED, "mr_ragged/", dict(), 3),
    "levels1": (dict(SMALL2, levels=1), "mre_l1/", dict(), 2),
    "no_prior": (dict(SMALL2, prior_flows=0), "mre_np/", dict(), 2),
    "two_levels_rm_sr": (dict(SMALL2, levels=2, flows=1), "mre_l2/", dict(reverse_mode=True, super_resolution=True), 2),
    "bias": (dict(SMALL2, bias=True), "mre_b/", dict(), 2),
}
REFUSED = {"no_flow": (dict(SMALL2, prior_flows=0, flows=0), "mre_nf/", dict(), 2)}


def vs_module_inputs(name, arch, B, T):
    s = arch["hop_size"] // arch["n_group"]
    frames = (T + s - 1) // s
    x = torch.from_numpy(fill.uniform("mre/x/%s/%d" % (name, T), (B, T * arch["n_group"]), -1.0, 1.0)).to(DEV)
    h = torch.from_numpy(fill.normal("mre/h/%s/%d" % (name, T), (B, arch["n_mels"], frames))).to(DEV)
    return x, h


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(VS_MODULE))
def test_engine_vs_module_path(name, precision, monkeypatch, engine_on):
    set_precision(monkeypatch, precision)
    arch, tag, kw, B = VS_MODULE[name]
    m = build(arch, tag, memory_efficient=True, **kw)
    worst = [0.0, 0.0]
    for T in COLUMNS:
        x, h = vs_module_inputs(name, arch, B, T)
        keep = (x.clone(), h.clone())
        assert m._engine_route(x.detach(), h)[0] == "autograd is enabled"
        (z1, l1, x1, k1), (z0, l0, x0, k0) = both_paths(m, lambda: m(x, h) + m.reverse(x, h), monkeypatch)
        assert torch.equal(x, keep[0]) and torch.equal(h, keep[1])
        worst[0] = max(worst[0], float((z1 - z0).abs().max()), float((x1 - x0).abs().max()))
        for a, b in ((l1, l0), (k1, k0)):
            worst[1] = max(worst[1], float(((a - b).abs() / b.abs().clamp_min(1e-30)).max()))
            check_logdet(a, b, x.size(1))
        assert torch.equal(z1, z0) and torch.equal(x1, x0), (name, precision, T)      # (measured bit-equal in every mode: see the head of the file)
        assert z1.shape == x.shape and l1.shape == (B,) and bool(torch.isfinite(z1).all()) and bool(torch.isfinite(x1).all())
    print("%s %s: engine vs module path: max |dx| %.3e, max relative |dlogdet| %.3e" % (name, precision, worst[0], worst[1]))


def test_refused_configuration_takes_the_module_path(monkeypatch, engine_on):
    arch, tag, kw, B = REFUSED["no_flow"]
    m = cm.MRWaveGlow(memory_efficient=True, **kw, **arch).to(DEV).eval()
    x, h = vs_module_inputs("no_flow", arch, B, 13)
    p0 = passes()
    with torch.no_grad():
        assert m._engine_route(x, h)[0] == "wg_mr_check: code -3"
        z, ld = m(x, h)
        xr, _ = m.reverse(z, h)
    assert passes() == p0 and ld == 0                                   # no flow: the module's logdet is the integer 0
    assert torch.equal(z.cpu(), r64.analysis64(x.cpu(), arch["n_group"], arch["levels"]))
    assert float((xr - x).abs().max()) <= 8 * r64.U32 * float(x.abs().max())


# ---- 3. the plane kernels alone --------------------------------------------------------------------------------------------------
def dev(name, shape):
    return torch.from_numpy(fill.normal(name, shape)).to(DEV)


def plane_geo(T, halo):
    H, P = C.c_int(0), C.c_int(0)
    check(_lib.lib().wg_mr_plane_geo(T, halo, C.byref(H), C.byref(P)), "wg_mr_plane_geo")
    assert H.value >= max(halo, 16) and H.value % 16 == 0 and P.value == 2 * H.value + (T + 127) // 128 * 128
    return H.value, P.value


def plane(B, rows, P, value):
    return torch.full((B, rows, P), value, dtype=torch.float32, device=DEV)


def to_plane(t, rows, ch0, H, P, value=0.0):
    p = plane(t.size(0), rows, P, value)
    p[:, ch0:ch0 + t.size(1), H:H + t.size(2)] = t
    return p


def assert_owned(p, ch0, n, H, T, want, value, what):
    """rows [ch0, ch0 + n) x columns [H, H + T) hold `want` bit for bit; every other element is still `value` (NaN or zero)"""
    assert torch.equal(p[:, ch0:ch0 + n, H:H + T].cpu(), want), what
    rest = p.clone()
    rest[:, ch0:ch0 + n, H:H + T] = value
    assert bool(torch.isnan(rest).all()) if value != value else bool((rest == 0).all()), what


def run_split(audio, src, B, T, halo, c, diff, d0, cond, avg, a0):
    check(_lib.lib().wg_mr_plane_split(engine._p(audio), engine._p(src), 0 if src is None else src.size(1), B, T, halo, c, engine._p(diff),
                                       diff.size(1), d0, engine._p(cond), cond.size(1), engine._p(avg), 0 if avg is None else avg.size(1), a0,
                                       engine._stream(DEV)), "wg_mr_plane_split")


def run_merge(avg, diff, d0, B, T, halo, c, out, audio):
    check(_lib.lib().wg_mr_plane_merge(engine._p(avg), avg.size(1), engine._p(diff), diff.size(1), d0, B, T, halo, c, engine._p(out),
                                       0 if out is None else out.size(1), engine._p(audio), engine._stream(DEV)), "wg_mr_plane_merge")


@pytest.mark.parametrize("T", COLUMNS)
def test_plane_split_and_merge_are_bit_equal_and_leave_the_rest(T):
    for B, c, halo, value in [(1, 2, 4, NAN), (2, 4, 4, 0.0), (2, 8, 16, NAN), (3, 16, 8, NAN), (1, 32, 130, 0.0)]:
        H, P = plane_geo(T, halo)
        half, rows_x, rows_c, d0, a0 = c // 2, c + 16, c // 2 + 9, 3, c // 2 + 5
        x = dev("mrp/x%d" % c, (B, c, T))
        wd, wa = (t.float() for t in r64.haar_split64(x.cpu().double()))
        audio = x.transpose(1, 2).contiguous().view(B, T * c)            # the audio's layout: [B, T, c]
        keep = audio.clone()
        src = to_plane(x, c + 3, 0, H, P)
        for from_audio in (True, False):
            for with_avg in (True, False):
                what = (T, B, c, from_audio, with_avg)
                diff, cond = plane(B, rows_x, P, value), plane(B, rows_c, P, value)
                avg = plane(B, rows_x, P, value) if with_avg else None
                run_split(audio if from_audio else None, None if from_audio else src, B, T, halo, c, diff, d0, cond, avg, a0)
                assert_owned(diff, d0, half, H, T, wd, value, what)
                assert_owned(cond, 0, half, H, T, wa, value, what)
                if with_avg:
                    assert_owned(avg, a0, half, H, T, wa, value, what)
        assert torch.equal(audio, keep) and torch.equal(src[:, :c, H:H + T], x)
        # merge: into the next plane, and (the last merge) into the audio; avg and diff as the split left them
        avg_p, diff_p = to_plane(wa.to(DEV), rows_c, 0, H, P), to_plane(wd.to(DEV), rows_x, d0, H, P)
        want = r64.haar_merge64(wa.double(), wd.double()).float()
        out = plane(B, c + 5, P, value)
        run_merge(avg_p, diff_p, d0, B, T, halo, c, out, None)
        assert_owned(out, 0, c, H, T, want, value, (T, B, c, "merge"))
        for shift in (0, 1):                                             # shift 1: an audio buffer off 16-byte alignment, the scalar walk
            buf = torch.full((B * T * c + 2,), NAN, device=DEV)
            flat = buf[shift:shift + B * T * c].view(B, T * c)
            run_merge(avg_p, diff_p, d0, B, T, halo, c, None, flat)
            assert torch.equal(flat.view(B, T, c).transpose(1, 2).cpu(), want), (T, B, c, "merge to audio", shift)
            assert bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + B * T * c:]).all())
            assert float((flat - audio).abs().max()) <= 4 * r64.U32 * float(audio.abs().max())
            diff, cond = plane(B, rows_x, P, value), plane(B, rows_c, P, value)      # ... and the split reading that buffer back
            run_split(flat, None, B, T, halo, c, diff, d0, cond, None, 0)
            wd2, wa2 = (t.float() for t in r64.haar_split64(want.double()))
            assert_owned(diff, d0, half, H, T, wd2, value, (T, B, c, "split", shift))
            assert_owned(cond, 0, half, H, T, wa2, value, (T, B, c, "split", shift))


@pytest.mark.parametrize("T", COLUMNS)
def test_plane_upsample_fills_every_plane_once(T):
    for s, n_mels, B, halo, value in [(32, 80, 2, 4, NAN), (5, 7, 3, 8, 0.0), (1, 3, 1, 4, NAN), (4, 1, 2, 130, NAN)]:
        F = (T + s - 1) // s + 1                                         # one trailing frame the cut may or may not reach
        H, P = plane_geo(T, halo)
        h = dev("mrp/h%d" % n_mels, (B, n_mels, F))
        keep = h.clone()
        same = engine.mr_upsample(h, s, T).cpu()                          # wg_mr_upsample: the arithmetic this kernel repeats
        h64 = h.cpu().double()
        bound = r64.fma_bound(2, torch.einsum("tf,bmf->bmt", r64.upsample_weights64(s, F, T), h64.abs()))
        assert bool(((same.double() - r64.upsample64(h64, s, T)).abs() <= bound).all())
        for nd in (1, 3):
            rows = [n_mels + 2, n_mels + 21, n_mels + 8][:nd]
            ch0 = [0, 16, 3][:nd]
            planes = [plane(B, r, P, value) for r in rows]
            ptrs = (C.c_void_p * nd)(*[p.data_ptr() for p in planes])
            check(_lib.lib().wg_mr_plane_upsample(engine._p(h), B, n_mels, F, s, T, halo, nd, ptrs, (C.c_int * nd)(*rows), (C.c_int * nd)(*ch0),
                                                  engine._stream(DEV)), "wg_mr_plane_upsample")
            for p, c0 in zip(planes, ch0):
                assert_owned(p, c0, n_mels, H, T, same, value, (T, s, n_mels, nd))
        assert torch.equal(h, keep)
    assert _lib.lib().wg_mr_plane_upsample(engine._p(h), B, n_mels, 1, 1, 2, 4, 1, ptrs, (C.c_int * 1)(4), (C.c_int * 1)(0), None) == -2       # T > F s


# ---- 4. / 5. determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mr_small", "mr_ragged"])
def test_two_fresh_engines_give_the_same_bits(name, monkeypatch, engine_on):
    ref = mrg.load(name, GOLD)
    runs = []
    for _ in range(2):
        m, arch = fixture_model(name)
        B, N, frames = mrg.SHAPES[mrg.INPUT_TAG[name]]
        audio, h = mrg.inputs(mrg.INPUT_TAG[name], B, N, arch["n_mels"], frames)
        x, ht, z = torch.from_numpy(audio).to(DEV), torch.from_numpy(h).to(DEV), torch.from_numpy(ref["z"]).to(DEV)
        p0 = passes()
        with torch.no_grad():
            runs.append(m(x, ht) + m.reverse(z, ht) + m.reverse(z, ht))
        assert passes() - p0 == 3
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][2], runs[0][4]) and torch.equal(runs[0][3], runs[0][5])      # ... and a second call on the same engine


# ---- 6. graphs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rmode", [False, True])
def test_graph_replay_repack_and_auto_capture(rmode, monkeypatch):
    monkeypatch.delenv("WG_MR_ENGINE", raising=False)
    m = build(SMALL2, "mre/", memory_efficient=True, reverse_mode=rmode)
    x, h = vs_module_inputs("graph", SMALL2, 2, 260)
    synth = m.reverse                                                  # towards the audio as the caller sees it: the captured direction

    def run(graphs):
        if graphs is None:
            monkeypatch.delenv("WG_GRAPHS", raising=False)
        else:
            monkeypatch.setenv("WG_GRAPHS", graphs)
        with torch.no_grad():
            return synth(x, h)

    a, b = run("0"), run("0")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and len(m.mr_engine()._graphs) == 0
    p0 = passes()
    g1, g2 = run("1"), run("1")                                        # captured, then replayed
    assert len(m.mr_engine()._graphs) == 1
    assert passes() - p0 == 2                                          # the warm-up and the capture; a replay calls nothing
    for g in (g1, g2):
        assert torch.equal(g[0], a[0]) and torch.equal(g[1], a[1])
    with torch.no_grad():                                              # the other direction is never captured
        run_other = m(x, h)
    assert len(m.mr_engine()._graphs) == 1 and passes() - p0 == 3 and bool(torch.isfinite(run_other[0]).all())
    with torch.no_grad():                                              # weights changed in place: re-packed into the same buffer
        m.prior_WNs[1].F.end.weight.mul_(1.5)
        m.invconv1x1_list[0][1].weight.mul_(1.1)
    g3 = run("1")
    assert len(m.mr_engine()._graphs) == 1 and passes() - p0 == 3
    d = run("0")
    assert not torch.equal(d[0], a[0]) and not torch.equal(d[1], a[1])
    assert torch.equal(g3[0], d[0]) and torch.equal(g3[1], d[1])
    # auto: a small call is captured on its third occurrence
    m2 = build(SMALL2, "mre/", memory_efficient=True, reverse_mode=rmode)
    synth = m2.reverse
    want = None
    for n in (1, 2, 3, 4):
        out = run(None)
        want = out if want is None else want
        assert len(m2.mr_engine()._graphs) == (0 if n < 3 else 1), n
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


# ---- 7. round trip and sampling --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mr_small", "mr_small_rm", "mr_small_sr", "mr_ragged"])
def test_round_trip_and_infer(name, monkeypatch, engine_on):
    m, arch = fixture_model(name)
    B, N, frames = mrg.SHAPES[mrg.INPUT_TAG[name]]
    audio, h = mrg.inputs(mrg.INPUT_TAG[name], B, N, arch["n_mels"], frames)
    x, ht = torch.from_numpy(audio).to(DEV), torch.from_numpy(h).to(DEV)
    p0 = passes()
    with torch.no_grad():
        z, ld = m(x, ht)
        xr, ldr = m.reverse(z, ht)
    assert float((xr - x).abs().max()) < 1e-4
    assert float((ld + ldr).abs().max()) <= 1e-4 * float(ld.abs().max())
    out = m.infer(ht, sigma=0.6)
    assert out.shape == (B, frames * arch["hop_size"]) and bool(torch.isfinite(out).all())
    one = m.infer(ht[0])
    assert one.shape == (frames * arch["hop_size"],) and bool(torch.isfinite(one).all())
    assert passes() - p0 == 4
    # a model left in train(): infer stays on the module path
    m.train()
    assert m.infer(ht, sigma=0.6).shape == out.shape and passes() - p0 == 4


def test_route_sees_what_changes_behind_its_caches(monkeypatch, engine_on):
    """The route reads the module list from the cached slots and skips the parameters' dtype / device scan while their (address,
    version) key is the packed one: a sub-module put in train(), a block swapped in, and parameters converted after a served call must
    all still be seen."""
    m = build(SMALL2, "mre/", memory_efficient=True)
    x, h = vs_module_inputs("route", SMALL2, 2, 13)
    with torch.no_grad():
        z, _ = m(x, h)
        assert m._engine_route(x, h)[0] is None and m.mr_engine().packed.key == m._engine_route(x, h)[2]     # served, and packed
        m.WNs_list[1][0].F.layers[1].train()
        assert m._engine_route(x, h)[0] == "a module is in train()"
        m.eval()
        assert m._engine_route(x, h)[0] is None
        other = build(SMALL2, "mre_other/", memory_efficient=True)
        m.prior_WNs[1] = other.prior_WNs[1]                             # a block swapped in: the slots re-resolve, the weights re-pack
        p0 = passes()
        z2, _ = m(x, h)
        monkeypatch.setenv("WG_MR_ENGINE", "0")
        z3, _ = m(x, h)
        monkeypatch.delenv("WG_MR_ENGINE")
        assert passes() - p0 == 1 and not torch.equal(z2, z) and torch.equal(z2, z3)
        m.prior_WNs[1].train()
        assert m._engine_route(x, h)[0] == "a module is in train()"
        m.eval()
        m.half()
        assert m._engine_route(x, h)[0] == "parameters are not float32"
        m.float()
        p0 = passes()
        z4, _ = m(x, h)
        monkeypatch.setenv("WG_MR_ENGINE", "0")
        z5, _ = m(x, h)
        assert passes() - p0 == 1 and torch.equal(z4, z5) and not torch.equal(z4, z2)      # re-packed: the weights went through fp16


# ---- 8. the shipped architecture once --------------------------------------------------------------------------------------------
_FULL = {}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_shipped_architecture_engine_vs_module_path(precision, monkeypatch, engine_on):
    set_precision(monkeypatch, precision)
    arch = mrg.ARCH_FULL
    m = cm.MRWaveGlow(memory_efficient=True, **arch)
    if not _FULL:
        _FULL.update({k: torch.from_numpy(np.asarray(v)) for k, v in mrg.param_values(m, "mr_full/").items()})
    m.load_state_dict(_FULL)
    m = m.to(DEV).eval()
    frames = 8
    x, h = mrg.inputs("mre_full", 1, frames * arch["hop_size"], arch["n_mels"], frames)
    x, h = torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV)
    (z1, l1, x1, k1), (z0, l0, x0, k0) = both_paths(m, lambda: m(x, h) + m.reverse(x, h), monkeypatch)
    dz, dx = float((z1 - z0).abs().max()), float((x1 - x0).abs().max())
    print("shipped %s: engine vs module path: max |dz| %.3e, max |dx| %.3e" % (precision, dz, dx))
    assert bool(torch.isfinite(z1).all()) and bool(torch.isfinite(x1).all())
    assert dz == 0.0 and dx == 0.0                                      # (bit-equal, as at the small shapes)
    check_logdet(l1, l0, x.size(1))
    check_logdet(k1, k0, x.size(1))
