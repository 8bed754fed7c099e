"""MRWaveGlow on the CPU side (no kernel launches): construction from the shipped config, the reference's state-dict contract, the
fixture recipe, the float64 restatements the GPU tests measure with (golden/mr_ref64.py) against the reference's own class, what every
wg_mr_* entry point answers before it launches, and the shapes the module refuses."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fill
import mr_ref64 as r64
import constant_memory_waveglow_amd as cm
from constant_memory_waveglow_amd import WgError, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# configs/mr_waveglow_LJ_speech.json upstream, "arch"
SHIPPED = {"type": "MRWaveGlow", "args": {"prior_flows": 4, "n_group": 8, "hop_size": 256, "n_mels": 80, "memory_efficient": True,
                                          "reverse_mode": False, "dilation_channels": 256, "residual_channels": 256,
                                          "skip_channels": 256, "depth": 8, "radix": 3, "bias": False}}
SMALL_WN = dict(dilation_channels=32, residual_channels=32, skip_channels=32, depth=2, radix=3, bias=False)


def test_get_instance_builds_the_shipped_config():
    m = cm.get_instance(cm, SHIPPED)
    assert isinstance(m, cm.MRWaveGlow)
    assert len(m.state_dict()) == 456
    assert sum(p.numel() for p in m.parameters()) == 53_735_520
    assert m.z_split_sizes == [4, 2, 2] and m.upsample_factor == 32
    assert [(b.F.in_chs, b.F.aux_chs) for lvl in m.WNs_list for b in lvl] == [(2, 84)] * 4 + [(1, 82)] * 4
    assert [(b.F.in_chs, b.F.aux_chs) for b in m.prior_WNs] == [(1, 80)] * 4
    # upstream's quirk: the level 1x1 convs are always memory-efficient and never in reverse mode
    rm = cm.MRWaveGlow(2, 8, 256, 80, False, reverse_mode=True, flows=1, **SMALL_WN)
    assert all(c._memory_efficient and not c._reverse_mode for lvl in rm.invconv1x1_list for c in lvl)
    assert all(not c._memory_efficient and c._reverse_mode for c in rm.prior_invconv1x1)
    assert all(not b._memory_efficient and b._reverse_mode for lvl in rm.WNs_list for b in lvl)


@pytest.mark.reference
@pytest.mark.parametrize("over", [dict(), dict(levels=4, n_group=16, **SMALL_WN), dict(super_resolution=True, **SMALL_WN)],
                         ids=["shipped", "levels4", "sr"])
def test_state_dict_matches_reference(over):
    import importlib
    import ref_shim
    ref_shim.load()
    Ref = importlib.import_module("model.mr_waveglow").MRWaveGlow
    args = dict(SHIPPED["args"], **over)
    ours, ref = cm.MRWaveGlow(**args), Ref(**args)
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    assert [n for n, _ in ours.named_parameters()] == [n for n, _ in ref.named_parameters()]
    ours.load_state_dict(b, strict=True)                            # interchangeable both ways
    ref.load_state_dict(ours.state_dict(), strict=True)


@pytest.mark.reference
@pytest.mark.timeout(600)
def test_recipe_regenerates_the_small_fixtures_bit_for_bit(tmp_path):
    small = ["mr_small", "mr_small_nme", "mr_small_rm", "mr_small_sr", "mr_ragged"]
    env = dict(os.environ, WG_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_mrwaveglow.py")], env=env, cwd=str(tmp_path), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    committed = sorted(glob.glob(os.path.join(GOLD, "mr", "*.npz")))
    assert [os.path.basename(f) for f in committed] == sorted(["model_%s%s.npz" % (n, w) for n in small for w in ("", "_w")] +
                                                              ["model_mr_full.npz"])
    assert max(os.path.getsize(f) for f in committed) <= 1 << 20           # (the repository's limit for a committed file)
    for f in committed:
        if f.endswith("model_mr_full.npz"):
            continue
        a, b = np.load(f), np.load(os.path.join(str(tmp_path), os.path.basename(f)))
        assert sorted(a.files) == sorted(b.files), f
        for k in a.files:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (f, k)
    import make_golden_mrwaveglow as mrg
    for n in small:                                 # every gradient of every small case is there, in full
        arrays = mrg.load(n)
        arch, _, me, rmode, sr = mrg.CASES[n]
        ours = cm.MRWaveGlow(memory_efficient=me, reverse_mode=rmode, super_resolution=sr, **arch)
        shapes = {"grad::" + k: tuple(p.shape) for k, p in ours.named_parameters()}
        assert {k: tuple(v.shape) for k, v in arrays.items() if k.startswith("grad::")} == shapes, n


# ---- the float64 yardstick of the GPU tests ----------------------------------------------------------------------------------------
@pytest.mark.reference
@pytest.mark.parametrize("n_group,levels,hop,frames,T", [(8, 3, 256, 8, 256), (16, 4, 80, 3, 13), (8, 2, 8, 5, 5), (4, 1, 12, 2, 6)])
def test_ref64_matches_the_reference_class(n_group, levels, hop, frames, T):
    """The reference's own MRWaveGlow without any flow (prior_flows = flows = 0) is the Haar analysis and the packing alone, its reverse
    the unpacking and the merges; `_upsample_h` is its upsampling.  float64 on both sides: 1e-12 on O(1) values."""
    import importlib
    import ref_shim
    ref_shim.load()
    Ref = importlib.import_module("model.mr_waveglow").MRWaveGlow
    ref = Ref(0, n_group, hop, 7, False, levels=levels, flows=0)
    B = 3
    x = torch.from_numpy(fill.uniform("r64/x", (B, T * n_group))).double()
    h = torch.from_numpy(fill.normal("r64/h", (B, 7, frames))).double()
    with torch.no_grad():
        z_ref, _ = ref.forward_computation(x, h)
        x_ref, _ = ref.reverse_computation(z_ref.clone(), h)
        y_ref = ref._upsample_h(h)
    s = hop // n_group
    assert float((r64.analysis64(x, n_group, levels) - z_ref).abs().max()) < 1e-12
    assert float((r64.synthesis64(z_ref, n_group, levels) - x_ref).abs().max()) < 1e-12
    assert float((x_ref - x).abs().max()) < 1e-12
    assert y_ref.shape == (B, 7, frames * s)
    assert float((r64.upsample64(h, s, T) - y_ref[..., :T]).abs().max()) < 1e-12
    # the integer form of the weights (the kernels' definition) is the same map
    W = r64.upsample_weights64(s, frames, T)
    assert float((torch.einsum("tf,bmf->bmt", W, h) - y_ref[..., :T]).abs().max()) < 1e-12
    assert float((W.sum(1) - 1).abs().max()) < 1e-15
    parts = r64.unpack64(z_ref, n_group, r64.split_sizes(n_group, levels))
    assert [p.size(1) for p in parts] == r64.split_sizes(n_group, levels) and torch.equal(r64.pack64(parts), z_ref)


# ---- the entry points before any launch --------------------------------------------------------------------------------------------
EINVAL, ESHAPE, EUNSUPPORTED = -1, -2, -3


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy non-NULL addresses and no device in this process: a launch would answer WG_ELAUNCH (-4), a dereference would crash."""
    L = _lib.lib()
    p, null = C.c_void_p(4096), C.c_void_p(0)

    def split(x=p, s=(64, 8, 1), B=2, c=8, T=8, mode=0, diff=p, avg=p, cond=null, rows=0):
        return L.wg_mr_haar_split(x, s[0], s[1], s[2], B, c, T, mode, diff, avg, cond, rows, null)

    for bad in (dict(x=null), dict(diff=null), dict(avg=null), dict(B=0), dict(c=0), dict(c=7), dict(T=0), dict(mode=2), dict(mode=-1),
                dict(s=(-64, 8, 1)), dict(s=(64, -8, 1)), dict(s=(64, 8, -1)), dict(cond=p, rows=3)):
        assert split(**bad) == EINVAL, bad
    assert split(B=1 << 20, c=2, T=1 << 22) == EUNSUPPORTED                       # more blocks than a grid holds

    def merge(avg=p, avg2=null, rows2=0, diff=p, B=2, c=8, T=8, mode=0, out=p, s=(64, 8, 1)):
        return L.wg_mr_haar_merge(avg, avg2, rows2, diff, B, c, T, mode, out, s[0], s[1], s[2], null)

    for bad in (dict(avg=null), dict(diff=null), dict(out=null), dict(B=-1), dict(c=1), dict(c=7), dict(T=0), dict(mode=3),
                dict(s=(64, 8, -1)), dict(s=(64, 0, 1)), dict(s=(64, 8, 0)), dict(avg2=p, rows2=3)):
        assert merge(**bad) == EINVAL, bad
    assert merge(B=1 << 20, c=2, T=1 << 22) == EUNSUPPORTED

    def up(h=p, head=null, B=2, n_mels=80, F=8, s=32, T=256, out=p, rows=84, r0=4):
        return L.wg_mr_upsample(h, head, B, n_mels, F, s, T, out, rows, r0, null)

    for bad in (dict(h=null), dict(out=null), dict(B=0), dict(n_mels=0), dict(F=0), dict(s=0), dict(T=0), dict(rows=83), dict(r0=-1),
                dict(head=p, r0=0, rows=80)):
        assert up(**bad) == EINVAL, bad
    assert up(T=257) == ESHAPE and up(F=1, s=5, T=6) == ESHAPE                    # more columns than the frames upsample to
    assert up(F=1 << 20, s=1 << 11, T=5) == EUNSUPPORTED                          # positions beyond int arithmetic

    def upb(dout=p, rows=84, r0=4, B=2, n_mels=80, F=8, s=32, T=256, dh=p):
        return L.wg_mr_upsample_backward(dout, rows, r0, B, n_mels, F, s, T, dh, null)

    for bad in (dict(dout=null), dict(dh=null), dict(B=0), dict(n_mels=0), dict(F=0), dict(s=0), dict(T=0), dict(rows=83), dict(r0=-1)):
        assert upb(**bad) == EINVAL, bad
    assert upb(T=257) == ESHAPE and upb(F=1 << 20, s=1 << 11, T=5) == EUNSUPPORTED

    for fn in (L.wg_mr_pack, L.wg_mr_unpack):
        call = lambda src=p, B=2, c=4, T=8, n_group=8, off=0, dst=p: fn(src, B, c, T, n_group, off, dst, null)
        for bad in (dict(src=null), dict(dst=null), dict(B=0), dict(c=0), dict(T=0), dict(n_group=0), dict(off=-1), dict(off=5),
                    dict(c=9)):
            assert call(**bad) == EINVAL, bad
        assert call(B=1 << 20, T=1 << 20) == EUNSUPPORTED


# ---- the module's own refusals -----------------------------------------------------------------------------------------------------
def _small(**over):
    kw = dict(prior_flows=1, n_group=8, hop_size=256, n_mels=80, memory_efficient=True, flows=1, **SMALL_WN)
    kw.update(over)
    return cm.MRWaveGlow(**kw)


def test_module_refuses_bad_shapes_and_the_cpu_before_any_launch():
    m = _small()
    with pytest.raises(WgError, match="no CPU fallback"):
        m(torch.zeros(2, 2048), torch.zeros(2, 80, 8))
    with pytest.raises(WgError, match="no CPU fallback"):
        m.reverse(torch.zeros(2, 2048), torch.zeros(2, 80, 8))
    with pytest.raises(WgError, match="multiple of n_group"):
        m(torch.zeros(2, 2047), torch.zeros(2, 80, 8))
    with pytest.raises(WgError, match="7 frames upsample to 224 columns, the audio has 256"):
        m(torch.zeros(2, 2048), torch.zeros(2, 80, 7))
    with pytest.raises(WgError, match="expects"):
        m(torch.zeros(2, 2048), torch.zeros(2, 79, 8))
    with pytest.raises(WgError, match="expects"):
        m(torch.zeros(2, 8, 256), torch.zeros(2, 80, 8))
    with pytest.raises(WgError, match="no CPU fallback"):
        m.infer(torch.zeros(80, 8))


@pytest.mark.parametrize("n_group,levels", [(8, 4), (12, 3), (6, 2), (10, 2), (7, 1)])
def test_constructor_refuses_channel_counts_that_do_not_split(n_group, levels):
    with pytest.raises(WgError, match="levels"):
        _small(n_group=n_group, levels=levels, hop_size=n_group * 4)
    assert _small(n_group=16, levels=4).z_split_sizes == [8, 4, 2, 2]
