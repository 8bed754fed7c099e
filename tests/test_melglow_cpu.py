"""MelGlow on the CPU side (no kernel launches): construction from the shipped config, the reference's state-dict contract, the
fixture recipe, the float64 restatements the GPU tests measure with (golden/mg_ref64.py) against the reference's own layer, the
shapes the LVC kernels refuse -- refused with a clear error before anything is launched -- on both sides of each limit, and what
wg_mg_gemm answers before it launches (workspace sizes, bad descriptors)."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mg_ref64 as r64
import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import WgError, _lib, engine, melglow as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# configs/melglow_LJ_speech.json upstream, "arch"
SHIPPED = {"type": "MelGlow", "args": {"flows": 12, "n_group": 8, "n_early_every": 4, "n_early_size": 2, "hop_size": 256, "n_mels": 80,
                                       "reverse_mode": False, "memory_efficient": True, "dilation_channels": 48, "residual_channels": 48,
                                       "skip_channels": 48, "depth": 7, "radix": 3, "predict_channels": 64, "predict_layers": 3,
                                       "bias": False}}


def test_get_instance_builds_the_shipped_config():
    m = cm.get_instance(cm, SHIPPED)
    assert isinstance(m, cm.MelGlow)
    assert len(m.state_dict()) == 732
    assert sum(p.numel() for p in m.parameters()) == 77_260_688
    assert m.z_split_sizes == [2, 2, 4]
    assert [blk.F.in_chs for blk in m.WNs] == [4] * 4 + [3] * 4 + [2] * 4
    assert not hasattr(m.WNs[0].F, "hip_dims")                     # the generic coupling path: recompute + BatchNorm semantics
    assert m.WNs[0].F.pred.end.weight.shape == (7 * 13824, 64, 1)


@pytest.mark.reference
def test_state_dict_matches_reference():
    import importlib
    import ref_shim
    ref_shim.load()
    Ref = importlib.import_module("model.melglow").MelGlow
    args = dict(SHIPPED["args"])
    ours, ref = cm.MelGlow(**args), Ref(**args)
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    assert [n for n, _ in ours.named_parameters()] == [n for n, _ in ref.named_parameters()]
    ours.load_state_dict(b)                                         # interchangeable both ways
    ref.load_state_dict(ours.state_dict())


@pytest.mark.reference
@pytest.mark.timeout(900)
def test_recipe_regenerates_the_fixtures(tmp_path):
    env = dict(os.environ, WG_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_melglow.py"), "mg_small", "mg_small_nme", "mg_small_rm", "mg_ragged",
                        "mg_full"],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    committed = sorted(glob.glob(os.path.join(GOLD, "mg", "*.npz")))
    assert [os.path.basename(f) for f in committed] == ["model_mg_full.npz", "model_mg_ragged.npz", "model_mg_small.npz",
                                                        "model_mg_small_nme.npz", "model_mg_small_rm.npz"]
    assert max(os.path.getsize(f) for f in committed) == os.path.getsize(os.path.join(GOLD, "mg", "model_mg_full.npz"))
    for f in committed:
        a, b = np.load(f), np.load(os.path.join(str(tmp_path), os.path.basename(f)))
        assert sorted(a.files) == sorted(b.files), f
        for k in a.files:
            x, y = a[k], b[k]
            # autograd's CPU convolutions sum in thread order: gradients (and the shipped size's summaries) within 1e-6 of the max
            if x.dtype.kind not in "fc" or not (k.startswith(("grad", "dh")) or "full" in f):
                assert np.array_equal(x, y), (f, k)
            elif x.size:
                scale = max(float(np.abs(x).max()), 1e-9)
                assert float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) <= 1e-6 * scale + 1e-9, (f, k)


def _wn(**over):
    kw = dict(in_channels=4, aux_channels=80, depth=7, dilation_channels=16, residual_channels=16, skip_channels=16, predict_channels=8,
              predict_layers=1, radix=3, bias=False)
    kw.update(over)
    return cm.WN_LVC(**kw)


@pytest.mark.parametrize("over,T,F,what", [
    (dict(radix=2), 256, 8, "radix 2"),                     # even kernel
    (dict(), 250, 8, "T 250"),                              # T not a multiple of the frames
    (dict(), 8 * 256, 8, "8 frames"),                      # 256 columns per frame: wider than the kernels serve
    (dict(dilation_channels=160, residual_channels=160, skip_channels=160), 256, 8, "res 160"),
    (dict(bias=True), 256, 8, "bias=True"),
])
def test_unsupported_shapes_are_refused_before_any_launch(over, T, F, what):
    wn = _wn(**over)
    x, y = torch.zeros(2, 4, T), torch.zeros(2, 80, F)          # CPU tensors: the shape check must come before the device check
    with pytest.raises(WgError) as e:
        wn(x, y)
    assert what in str(e.value) and "CPU" not in str(e.value)


def test_layer_and_predictor_refuse_bad_shapes_and_the_cpu():
    layer = mg.NonCausalLayerLVC(4, 16, 16, 16, 3, False)
    layer.apply(cm.add_weight_norms)
    with pytest.raises(WgError, match="weights"):
        layer(torch.zeros(2, 16, 64), torch.zeros(2, 2, 16, 16, 3))
    with pytest.raises(WgError, match="no CPU fallback"):
        layer(torch.zeros(2, 16, 64), torch.zeros(2, 2, 32, 16, 3))
    with pytest.raises(WgError, match="no CPU fallback"):
        mg.Predictor(80, 96, 16, 1, False, 7)(torch.zeros(2, 80, 3))
    with pytest.raises(WgError, match="expects"):
        mg.Predictor(80, 96, 16, 1, False, 7)(torch.zeros(2, 81, 3))


# ---- the float64 yardstick of the GPU tests ----------------------------------------------------------------------------------------
@pytest.mark.reference
@pytest.mark.parametrize("shape", r64.LAYER_SHAPES, ids=r64.shape_id)
def test_layer64_matches_the_reference_layer(shape):
    """layer64 / lvc_conv64 against upstream's NonCausalLayerLVC run in float64: 1e-12 absolute on O(1) values (float64 rounding over
    at most 256 terms)."""
    import importlib
    import ref_shim
    ref_shim.load()
    Ref = importlib.import_module("model.melglow").NonCausalLayerLVC
    R, D, S, radix, L, F, B, dilation, last = shape
    assert engine.lvc_check(_lib.WgLvcDims(R, D, radix, dilation), B, F * L, F) == 0
    xn, wn = r64.lvc_inputs("klayer/%d" % dilation, R, D, radix, L, F, B)
    x, w = torch.from_numpy(xn).double(), torch.from_numpy(wn).double()
    ref = Ref(dilation, D, R, S, radix, False, last_layer=last).double()
    wo = ref.W_o.weight.detach().squeeze(-1)
    with torch.no_grad():
        res_ref, skip_ref = ref(x, w)
        res, skip = r64.layer64(x, w, dilation, wo, R, last)
    assert 0.05 < float(skip_ref.abs().max()) < 50
    assert float((skip - skip_ref).abs().max()) < 1e-12
    assert (res is None and res_ref is None) if last else float((res - res_ref).abs().max()) < 1e-12


def test_lvc_inputs_scale_neighbouring_frames_apart():
    _, w = r64.lvc_inputs("klayer/1", 12, 10, 5, 25, 5, 3)
    rms = np.sqrt((w.astype(np.float64) ** 2).mean((2, 3, 4)))
    ratio = rms[:, 1:] / rms[:, :-1]
    assert np.all(np.maximum(ratio, 1 / ratio) > 2.0)


def test_gemm_expect_gathers_by_the_descriptor():
    """the float64 side of the wg_mg_gemm tests on a layout written out by hand: A [M][K] row-major, B k-blocks of K1 rows, padded"""
    M, N, K, K1 = 3, 4, 5, 2
    A, Bd = torch.arange(15.0).reshape(M, K), torch.arange(20.0).reshape(K, N) - 7
    B = torch.full((3, K1 * N + 1), float("nan"))                 # [k2][k1][n] + one unused element per block
    for k in range(K):
        B[k // K1, (k % K1) * N:(k % K1 + 1) * N] = Bd[k]
    offs = r64.gemm_offsets(M, N, K, 1, N, K1, (K, 1, K1, 0), (N, K1 * N + 1, 1, 0, 0), (N, 1, 0, 0))
    want, bound = r64.gemm_expect(A.reshape(-1), B.reshape(-1), torch.ones(12), offs, 2.0, -1.0, K, 1)
    assert torch.equal(want[0], 2.0 * (A.double() @ Bd.double()) - 1.0)
    assert torch.equal(bound[0], 8 * r64.U32 * (2.0 * (A.double().abs() @ Bd.double().abs()) + 1.0))


# ---- the limits of wg_lvc_check, both sides ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,D,radix,L,B,inside", [
    (4, 16, 3, 128, 1, True), (4, 17, 3, 121, 1, False),          # D L: 2048 / 2057
    (16, 4, 3, 128, 1, True), (17, 4, 3, 121, 1, False),          # R L
    (85, 4, 3, 8, 1, True), (86, 4, 3, 8, 1, False),              # R radix: 255 / 258 (256 and 257 have no odd radix with R <= 128)
    (4, 4, 3, 128, 1, True), (4, 4, 3, 129, 1, False),            # L
    (4, 128, 3, 16, 1, True), (4, 129, 3, 15, 1, False),          # D (129 x 15 = 1935: only the channel limit is crossed)
    (128, 4, 1, 16, 1, True), (129, 4, 1, 15, 1, False),          # R
    (4, 4, 3, 8, 65535, True), (4, 4, 3, 8, 65536, False),        # B
])
def test_lvc_check_limits_on_both_sides(R, D, radix, L, B, inside):
    F = 3
    rc = engine.lvc_check(_lib.WgLvcDims(R, D, radix, 2), B, F * L, F)
    assert rc == (0 if inside else -3)                            # WG_OK / WG_EUNSUPPORTED (include/wgflow.h)
    if not inside and B == 1:                                     # and the module says so before anything is launched
        layer = mg.NonCausalLayerLVC(2, D, R, 4, radix, False)
        layer.apply(cm.add_weight_norms)
        with pytest.raises(WgError, match="do not serve"):
            layer(torch.zeros(B, R, F * L), torch.zeros(B, F, 2 * D, R, radix))


# ---- wg_mg_gemm before any launch --------------------------------------------------------------------------------------------------
def _desc(M, N, K, batch=1, N1=None, K1=None):
    return _lib.WgMgGemmDesc(M, N, K, batch, N if N1 is None else N1, K if K1 is None else K1, K, 1, 0, M * K, N, 0, 1, 0, K * N,
                             N, 1, 0, M * N, 1.0, 1.0)


def test_gemm_workspace_sizes():
    ws = lambda *a, **k: int(_lib.lib().wg_mg_gemm_workspace_bytes(C.byref(_desc(*a, **k))))
    assert ws(48, 48, 1023) == 0                                  # K too short to cut
    assert ws(48, 48, 1024) == 2 * 48 * 48 * 4                    # two slices of 512
    assert ws(1024, 1024, 4096) == 0 and ws(64, 64, 4096, batch=256) == 0      # 256 tiles fill the chip
    assert ws(1024, 1023, 4096) == 0 and ws(1024, 960, 4096) > 0  # ... 256 with a partial tile, 240 without
    assert ws(48, 48, 22016) == 43 * 48 * 48 * 4 and ws(48, 48, 32769) == 64 * 48 * 48 * 4
    assert ws(8, 8, 1 << 20, batch=255) == 3 * 255 * 8 * 8 * 4    # slices x items stays far below the 65 535 layers of a grid
    assert ws(8, 8, 1 << 20, batch=65535) == 0
    for bad in [(0, 48, 4096), (48, 0, 4096), (48, 48, 0), (-1, 48, 4096), (48, -5, 4096), (48, 48, -4096)]:
        assert ws(*bad) == 0
    assert ws(48, 48, 4096, batch=0) == 0 and ws(48, 48, 4096, batch=-2) == 0
    assert _lib.lib().wg_mg_gemm_workspace_bytes(None) == 0


def test_gemm_refuses_before_any_launch():
    """Dummy non-NULL addresses: none of these paths dereferences or launches anything (no device in this process)."""
    L = _lib.lib()
    p, null = C.c_void_p(4096), C.c_void_p(0)
    call = lambda d, A=p, B=p, D=null, Cc=p, ws=null, n=0: L.wg_mg_gemm(C.byref(d), A, B, D, Cc, ws, n, null)
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -5
    cut = _desc(48, 48, 22016)
    need = int(L.wg_mg_gemm_workspace_bytes(C.byref(cut)))
    assert need > 0
    assert call(cut) == EWORKSPACE and call(cut, ws=null, n=need) == EWORKSPACE
    assert call(cut, ws=p, n=need - 1) == EWORKSPACE and call(cut, ws=p, n=0) == EWORKSPACE
    assert call(_desc(48, 48, 64, N1=0)) == EINVAL and call(_desc(48, 48, 64, K1=0)) == EINVAL
    assert call(_desc(48, 48, 64, N1=-3)) == EINVAL and call(cut, ws=p, n=need, A=null) == EINVAL
    small = _desc(48, 48, 64)
    assert call(small, A=null) == EINVAL and call(small, B=null) == EINVAL and call(small, Cc=null) == EINVAL
    assert L.wg_mg_gemm(None, p, p, null, p, null, 0, null) == EINVAL
    for bad in [(0, 48, 64), (48, 0, 64), (48, 48, 0)]:
        assert call(_desc(*bad)) == EINVAL
    assert call(_desc(48, 48, 64, batch=0)) == EINVAL
    assert call(_desc(8, 8, 64, batch=65536)) == EUNSUPPORTED
    assert call(_desc(8, 8, 4096, batch=65536), ws=p, n=1 << 40) == EUNSUPPORTED
    assert call(_desc(65536 * 64, 8, 8)) == EUNSUPPORTED           # more row tiles than a grid has layers
