"""The committed recipe reproduces the committed fixtures: `python tests/golden/make_golden.py` (no arguments = every fixture, in one
process) is run against the upstream reference into a scratch directory and every array is compared with tests/golden/*.npz.
Build container only (needs /root/reference); skipped where the reference is absent."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.reference
@pytest.mark.timeout(900)
def test_make_golden_main_regenerates_every_fixture(tmp_path):
    env = dict(os.environ, WG_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden.py")], env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # (the summary fixtures of the TIMED workloads -- one CPU training step of the reference at a benchmarked size -- are regenerated on
    # request only: `python make_golden.py c2_full wf_full wsr_full`; main() does not write them)
    on_request = {"model_wsr_full.npz", "model_c2_full.npz", "model_wf_full.npz"}
    committed = sorted(f for f in glob.glob(os.path.join(GOLD, "*.npz")) if os.path.basename(f) not in on_request)
    assert len(committed) == 24
    for f in committed:
        g = os.path.join(str(tmp_path), os.path.basename(f))
        assert os.path.exists(g), "main() did not write %s" % os.path.basename(f)
        a, b = np.load(f), np.load(g)
        assert sorted(a.files) == sorted(b.files), f
        # WaveFlow: Conv2d's backward sums in thread order (differences ~1e-8 of a tensor's max; the gradient of start.weight_v, exactly
        # zero in exact arithmetic, is rounding noise in both runs); everything else reproduces bit for bit
        # (the same for the gradient entries of the two stand-alone block fixtures: autograd through Conv1d / Conv2d; their forward entries are exact)
        base = os.path.basename(f)
        for k in a.files:
            x, y = a[k], b[k]
            grad_entry = base in ("block_layer.npz", "block_wn2d.npz") and k.split("/", 1)[-1].startswith(("dx", "dy", "grad"))
            exact = "model_wf" not in base and not grad_entry
            if x.dtype.kind not in "fc":
                assert np.array_equal(x, y), (f, k)
            elif exact:
                assert np.array_equal(x, y), (f, k)
            elif x.size:
                scale = max(float(np.abs(x).max()), 1e-9)
                assert float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) <= 1e-6 * scale + 1e-9, (f, k)


@pytest.mark.reference
@pytest.mark.timeout(900)
def test_make_golden_waveflow_regenerates_the_shape_fixtures(tmp_path):
    """tests/golden/wf/ (the WaveFlow heights and column counts of tests/test_gpu_waveflow_shapes.py) from its own recipe,
    `python tests/golden/make_golden_waveflow.py`: the eleven cases of fill.WF_SHAPE_FIXTURES and nothing else, each within the limit for
    a committed file, every array within the rule the WaveFlow fixtures above are held to."""
    sys.path.insert(0, GOLD)
    import fill
    env = dict(os.environ, WG_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_waveflow.py")], env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    committed = sorted(glob.glob(os.path.join(GOLD, "wf", "*.npz")))
    assert len(fill.WF_SHAPE_FIXTURES) == 11
    assert [os.path.basename(f) for f in committed] == sorted("model_%s.npz" % n for n in fill.WF_SHAPE_FIXTURES)
    assert max(os.path.getsize(f) for f in committed) <= 1 << 20
    for f in committed:
        g = os.path.join(str(tmp_path), os.path.basename(f))
        assert os.path.exists(g), "the recipe did not write %s" % os.path.basename(f)
        a, b = np.load(f), np.load(g)
        assert sorted(a.files) == sorted(b.files), f
        for k in a.files:
            x, y = a[k], b[k]
            assert x.shape == y.shape and x.dtype == y.dtype, (f, k)
            if x.dtype.kind not in "fc":
                assert np.array_equal(x, y), (f, k)
            elif x.size:                                   # (Conv2d's backward sums in thread order: ~1e-8 of a tensor's max)
                scale = max(float(np.abs(x).max()), 1e-9)
                assert float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) <= 1e-6 * scale + 1e-9, (f, k)
