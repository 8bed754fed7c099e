"""Generates the MelGlow fixtures tests/golden/mg/model_mg_*.npz by running the UPSTREAM REFERENCE's model/melglow.py (imported through
ref_shim) on the CPU, on deterministic inputs and parameters from fill.py.  Build container only.

    python tests/golden/make_golden_melglow.py            # the small cases and the ragged one (seconds)
    python tests/golden/make_golden_melglow.py mg_full    # the shipped configuration at 8 x 22 016, as a summary (minutes)

The fixtures live in their own directory, next to (not among) the WaveGlow / WaveFlow ones that make_golden.py regenerates.  Every
parameter is filled with non-trivial values: the reference zero-initialises each WN_LVC's `end`, which would make every coupling the
identity.  BatchNorm buffers start from keyed values too (running statistics away from 0 / 1, num_batches_tracked = 3), and the
fixtures record them after one training step: they moved once per transform call (twice per step when memory-efficient).
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.environ.get("WG_GOLDEN_OUT") or os.path.join(HERE, "mg")     # (tests regenerate into a scratch directory)
import fill       # noqa: E402
import ref_shim   # noqa: E402
from make_golden import _summ   # noqa: E402

ARCH_SMALL = dict(flows=4, n_group=8, n_early_every=2, n_early_size=2, hop_size=256, n_mels=80, dilation_channels=8,
                  residual_channels=8, skip_channels=8, depth=7, radix=3, predict_channels=4, predict_layers=1, bias=False)
ARCH_FULL = dict(flows=12, n_group=8, n_early_every=4, n_early_size=2, hop_size=256, n_mels=80, dilation_channels=48,
                 residual_channels=48, skip_channels=48, depth=7, radix=3, predict_channels=64, predict_layers=3, bias=False)
# ragged on purpose: L = hop / n_group = 25 columns per frame, T = 125 < the last dilations, R radix = 50, 2D = 12, R != D != S, 3 input
# channels in the last flow -- none of the LVC kernels' internal steps (24 / 16 / 32) divides anything here
ARCH_RAGGED = dict(flows=3, n_group=8, n_early_every=2, n_early_size=2, hop_size=200, n_mels=80, dilation_channels=6,
                   residual_channels=10, skip_channels=4, depth=8, radix=5, predict_channels=4, predict_layers=1, bias=False)
SHAPES = {"mg_small": (2, 8 * 256), "mg_ragged": (3, 1000), "mg_full": (8, 22016)}     # (batch, samples); frames = samples / hop
CASES = {                                                      # fixture -> (arch, parameter tag, memory_efficient, reverse_mode)
    "mg_small": (ARCH_SMALL, "mg_small/", True, False),
    "mg_small_nme": (ARCH_SMALL, "mg_small/", False, False),
    "mg_small_rm": (ARCH_SMALL, "mg_small/", True, True),
    "mg_ragged": (ARCH_RAGGED, "mg_ragged/", True, False),
}
INPUT_TAG = {"mg_small": "mg_small", "mg_small_nme": "mg_small", "mg_small_rm": "mg_small", "mg_ragged": "mg_ragged"}   # SHAPES / inputs key


def param_values(model, tag, arch):
    """name -> float32 / int64 array for every state-dict entry of a MelGlow module tree (reference's or this package's: same names)."""
    lvc_fan_in = arch["residual_channels"] * arch["radix"]
    sd = model.state_dict()
    out = {}
    for name, t in sd.items():
        shape = tuple(t.shape)
        key = tag + name
        if name.endswith("num_batches_tracked"):
            out[name] = np.array(3, np.int64)
        elif name.endswith("running_mean"):
            out[name] = fill.uniform(key, shape, -0.1, 0.1)
        elif name.endswith("running_var"):
            out[name] = fill.uniform(key, shape, 0.8, 1.2)
        elif ".invconv1x1." in "." + name:
            out[name] = fill.orthogonal(key, shape[0]).reshape(shape)
        elif name.endswith(".F.end.weight"):                           # the WN's output conv (zero upstream)
            out[name] = fill.normal(key, shape, 0.25 / np.sqrt(shape[1]))
        elif name.endswith("pred.end.weight"):                         # predicted kernels of std ~ 1 / sqrt(their fan-in)
            b = 3.0 / np.sqrt(shape[1] * lvc_fan_in)
            out[name] = fill.uniform(key, shape, -b, b)
        elif len(shape) == 1:                                         # BatchNorm affine
            out[name] = (fill.uniform(key, shape, 0.8, 1.2) if name.endswith("weight") else fill.uniform(key, shape, -0.1, 0.1))
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


def inputs(tag, B, N, n_mels, hop):
    return fill.uniform(tag + "/audio", (B, N), -1.0, 1.0), fill.normal(tag + "/mel", (B, n_mels, N // hop))


def load_reference():
    ref_shim.load()
    return importlib.import_module("model.melglow").MelGlow, ref_shim.load().WaveGlowLoss


def build(cls, arch, memory_efficient, reverse_mode, tag):
    m = cls(memory_efficient=memory_efficient, reverse_mode=reverse_mode, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in param_values(m, tag, arch).items()})
    return m


def small_fixture(name):
    arch, tag, me, rmode = CASES[name]
    MelGlow, Loss = load_reference()
    m = build(MelGlow, arch, me, rmode, tag)
    B, N = SHAPES[INPUT_TAG[name]]
    audio, h = inputs(INPUT_TAG[name], B, N, arch["n_mels"], arch["hop_size"])
    ht = torch.from_numpy(h).requires_grad_(True)
    z, ld = m(torch.tensor(audio), ht)               # (a tensor of its own: the memory-efficient blocks free and rebuild it)
    loss = Loss(fill.SIGMA)(z, ld)
    loss.backward()
    out = dict(z=z.detach().numpy(), logdet=ld.detach().numpy(), loss=np.float32(loss.item()), dh=ht.grad.numpy())
    for n, p in m.named_parameters():
        out["grad::" + n] = p.grad.numpy()
    for n, b in m.named_buffers():
        out["buf::" + n] = b.numpy().copy()
    m.eval()                                  # the inverse with the running statistics (a step in eval() moves no buffer)
    with torch.no_grad():
        xr, ldr = m.reverse(z.detach().clone(), ht.detach())
    out["x_inv_eval"], out["logdet_inv_eval"] = xr.numpy(), ldr.numpy()
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "model_%s.npz" % name), **out)
    print(name, "loss", out["loss"], "logdet", out["logdet"], "params", sum(p.numel() for p in m.parameters()))


def full_fixture():
    """The shipped configuration (configs/melglow_LJ_speech.json upstream) at batch 8 x 22 016, one memory-efficient training step, as
    a summary in the style of model_c2_full.npz."""
    MelGlow, Loss = load_reference()
    m = build(MelGlow, ARCH_FULL, True, False, "mg_full/")
    B, N = SHAPES["mg_full"]
    audio, h = inputs("mg_full", B, N, ARCH_FULL["n_mels"], ARCH_FULL["hop_size"])
    z, ld = m(torch.tensor(audio), torch.from_numpy(h))
    loss = Loss(fill.SIGMA)(z, ld)
    loss.backward()
    zz = z.detach().numpy()
    out = dict(z_head=zz[:, :256].copy(), z_tail=zz[:, -256:].copy(), z_item_norm=np.sqrt((zz.astype(np.float64) ** 2).sum(1)).astype(np.float32),
               logdet=ld.detach().numpy(), loss=np.float32(loss.item()))
    summ = [_summ(p.grad.numpy()) for _, p in m.named_parameters()]
    out["grad_norm"] = np.array([a for a, _, _ in summ], np.float32)
    out["grad_head"] = np.stack([b for _, b, _ in summ])
    out["grad_max"] = np.array([c for _, _, c in summ], np.float32)
    for n, b in m.named_buffers():
        if n.endswith("num_batches_tracked"):
            out["buf::" + n] = b.numpy().copy()
    rm = np.concatenate([b.numpy().ravel() for n, b in m.named_buffers() if n.endswith("running_mean")])
    rv = np.concatenate([b.numpy().ravel() for n, b in m.named_buffers() if n.endswith("running_var")])
    out["running_mean"], out["running_var"] = rm, rv
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "model_mg_full.npz"), **out)
    print("mg_full loss", out["loss"], "logdet", out["logdet"], "params", sum(p.numel() for p in m.parameters()),
          "state dict", len(m.state_dict()))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    for name in CASES:
        small_fixture(name)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        torch.manual_seed(0)
        torch.set_num_threads(8)
        for what in sys.argv[1:]:
            full_fixture() if what == "mg_full" else small_fixture(what)
    else:
        main()
