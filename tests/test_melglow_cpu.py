"""MelGlow on the CPU side (no kernel launches): construction from the shipped config, the reference's state-dict contract, the
fixture recipe, and the shapes the LVC kernels refuse -- refused with a clear error before anything is launched."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import WgError, melglow as mg

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
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_melglow.py"), "mg_small", "mg_small_nme", "mg_small_rm", "mg_full"],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    committed = sorted(glob.glob(os.path.join(GOLD, "mg", "*.npz")))
    assert [os.path.basename(f) for f in committed] == ["model_mg_full.npz", "model_mg_small.npz", "model_mg_small_nme.npz",
                                                        "model_mg_small_rm.npz"]
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
