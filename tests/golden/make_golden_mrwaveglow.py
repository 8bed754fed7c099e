"""Generates the MRWaveGlow fixtures tests/golden/mr/model_mr_*.npz by running the UPSTREAM REFERENCE's model/mr_waveglow.py (imported
through ref_shim) on the CPU, on deterministic inputs and parameters from fill.py.  Build container only.

    python tests/golden/make_golden_mrwaveglow.py            # the small cases and the ragged one (seconds)
    python tests/golden/make_golden_mrwaveglow.py mr_full    # the shipped configuration at 24 x 16 000, as a summary (minutes)

Each small case is two files, both with every array in full: model_<case>.npz (z, logdet, loss, dh, the eval-mode inverse and the
gradients) and model_<case>_w.npz (the gradients of the dilated convs, `layers.*.W.weight_v`, which are most of the bytes), so that no
committed file passes 1 MiB; `load(case)` reads the two as one.  The fixtures live in their own directory, next to (not among) the ones that make_golden.py regenerates.  Every parameter is filled with
non-trivial values: the reference zero-initialises each WN's `end`, which would make every coupling the identity.  The small cases run
on one thread, so that the reference's convolutions sum in one order and the recipe reproduces its fixtures bit for bit.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.environ.get("WG_GOLDEN_OUT") or os.path.join(HERE, "mr")     # (tests regenerate into a scratch directory)
import fill       # noqa: E402
import ref_shim   # noqa: E402
from make_golden import _summ   # noqa: E402

ARCH_SMALL = dict(prior_flows=2, flows=2, levels=3, n_group=8, hop_size=256, n_mels=80, dilation_channels=32, residual_channels=32,
                  skip_channels=32, depth=3, radix=3, bias=False)
# ragged on purpose: upsampling by 5 (weights that are no binary fractions), 3 frames = 15 columns cut to T = 13, four levels of a
# 16-channel group, the last dilation (4) times the kernel's reach (2) equal to more than half the 13 columns, R != D != S
ARCH_RAGGED = dict(prior_flows=1, flows=1, levels=4, n_group=16, hop_size=80, n_mels=7, dilation_channels=64, residual_channels=32,
                   skip_channels=96, depth=3, radix=5, bias=False)
# configs/mr_waveglow_LJ_speech.json upstream (levels and flows at their defaults)
ARCH_FULL = dict(prior_flows=4, n_group=8, hop_size=256, n_mels=80, dilation_channels=256, residual_channels=256, skip_channels=256,
                 depth=8, radix=3, bias=False)
SHAPES = {"mr_small": (2, 2048, 8), "mr_ragged": (3, 208, 3), "mr_full": (24, 16000, 63)}     # (batch, samples, mel frames)
CASES = {                                     # fixture -> (arch, parameter tag, memory_efficient, reverse_mode, super_resolution)
    "mr_small": (ARCH_SMALL, "mr_small/", True, False, False),
    "mr_small_nme": (ARCH_SMALL, "mr_small/", False, False, False),
    "mr_small_rm": (ARCH_SMALL, "mr_small/", True, True, False),
    "mr_small_sr": (ARCH_SMALL, "mr_small_sr/", True, False, True),
    "mr_ragged": (ARCH_RAGGED, "mr_ragged/", True, False, False),
}
INPUT_TAG = {"mr_small": "mr_small", "mr_small_nme": "mr_small", "mr_small_rm": "mr_small", "mr_small_sr": "mr_small",
             "mr_ragged": "mr_ragged"}                                                       # SHAPES / inputs key


def param_values(model, tag):
    """name -> float32 array for every state-dict entry of an MRWaveGlow module tree (reference's or this package's: same names), or of
    one of its blocks."""
    sd = model.state_dict()
    out = {}
    for name, t in sd.items():
        shape = tuple(t.shape)
        key = tag + name
        if "invconv1x1" in name:
            out[name] = fill.orthogonal(key, shape[0]).reshape(shape)
        elif ("." + name).endswith(".F.end.weight"):                           # the WN's output conv (zero upstream)
            out[name] = fill.normal(key, shape, 0.25 / np.sqrt(shape[1]))
        elif name.endswith("weight_g"):
            continue
        else:                                                         # conv weights and weight-norm directions
            b = 1.0 / np.sqrt(int(np.prod(shape[1:])))
            out[name] = fill.uniform(key, shape, -b, b)
    for name, t in sd.items():
        if name.endswith("weight_g"):
            v = out[name[:-1] + "v"].astype(np.float64)
            nrm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1))
            out[name] = (nrm * (1.0 + 0.2 * fill.uniform(tag + name, (v.shape[0],)).astype(np.float64))).astype(np.float32).reshape(t.shape)
    return out


def load(name, directory=None):
    """the arrays of a small case, from its two files, as one dict"""
    directory = directory or os.path.join(HERE, "mr")
    out = {}
    for f in ("model_%s.npz" % name, "model_%s_w.npz" % name):
        with np.load(os.path.join(directory, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def inputs(tag, B, N, n_mels, frames):
    return fill.uniform(tag + "/audio", (B, N), -1.0, 1.0), fill.normal(tag + "/mel", (B, n_mels, frames))


def load_reference():
    ns = ref_shim.load()
    return importlib.import_module("model.mr_waveglow").MRWaveGlow, ns.WaveGlowLoss


def build(cls, arch, memory_efficient, reverse_mode, super_resolution, tag):
    m = cls(memory_efficient=memory_efficient, reverse_mode=reverse_mode, super_resolution=super_resolution, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in param_values(m, tag).items()})
    return m


def _step(name):
    arch, tag, me, rmode, sr = CASES.get(name, (ARCH_FULL, "mr_full/", True, False, False))
    MRWaveGlow, Loss = load_reference()
    m = build(MRWaveGlow, arch, me, rmode, sr, tag)
    shape_tag = INPUT_TAG.get(name, name)
    B, N, frames = SHAPES[shape_tag]
    audio, h = inputs(shape_tag, B, N, arch["n_mels"], frames)
    ht = torch.from_numpy(h).requires_grad_(name != "mr_full")
    z, ld = m(torch.tensor(audio), ht)
    loss = Loss(fill.SIGMA)(z, ld)
    loss.backward()
    return m, z, ld, loss, ht, audio


def small_fixture(name):
    torch.set_num_threads(1)
    m, z, ld, loss, ht, audio = _step(name)
    out = dict(z=z.detach().numpy(), logdet=ld.detach().numpy(), loss=np.float32(loss.item()), dh=ht.grad.numpy())
    wide = {}                                     # the dilated convs' gradients, the bulk of the bytes, go to a file of their own
    for n, p in m.named_parameters():
        (wide if n.endswith(".W.weight_v") else out)["grad::" + n] = p.grad.numpy()
    m.eval()
    with torch.no_grad():
        xr, ldr = m.reverse(z.detach().clone(), ht.detach())
    out["x_inv_eval"], out["logdet_inv_eval"] = xr.numpy(), ldr.numpy()
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "model_%s.npz" % name), **out)
    np.savez_compressed(os.path.join(OUT, "model_%s_w.npz" % name), **wide)
    print(name, "loss", out["loss"], "logdet", out["logdet"], "params", sum(p.numel() for p in m.parameters()),
          "round trip", float(np.abs(out["x_inv_eval"] - audio).max()))


def full_fixture():
    """The shipped configuration at batch 24 x 16 000 with 63 frames (2016 upsampled columns cut to 2000), one memory-efficient
    training step, as a summary in the style of model_c2_full.npz."""
    torch.set_num_threads(8)
    m, z, ld, loss, _, _ = _step("mr_full")
    zz = z.detach().numpy()
    out = dict(z_head=zz[:, :256].copy(), z_tail=zz[:, -256:].copy(), z_item_norm=np.sqrt((zz.astype(np.float64) ** 2).sum(1)).astype(np.float32),
               logdet=ld.detach().numpy(), loss=np.float32(loss.item()))
    summ = [_summ(p.grad.numpy()) for _, p in m.named_parameters()]
    out["grad_norm"] = np.array([a for a, _, _ in summ], np.float32)
    out["grad_head"] = np.stack([b for _, b, _ in summ])
    out["grad_max"] = np.array([c for _, _, c in summ], np.float32)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "model_mr_full.npz"), **out)
    print("mr_full loss", out["loss"], "logdet", out["logdet"], "params", sum(p.numel() for p in m.parameters()),
          "state dict", len(m.state_dict()))


def main():
    for name in CASES:
        small_fixture(name)


if __name__ == "__main__":
    torch.manual_seed(0)
    if len(sys.argv) > 1:
        for what in sys.argv[1:]:
            full_fixture() if what == "mr_full" else small_fixture(what)
    else:
        main()
