"""Times one MelGlow training step at the shipped configuration (configs/melglow_LJ_speech.json upstream: 12 flows, 48 channels,
depth 7, predictor 64 x 3; batch 8 x 22 016, memory-efficient) on cuda:0 and prints one JSON line:

    {"ms_per_step": ..., "samples_per_s": ..., "lvc_us": {...}, "predictor_us": {...}, ...}

ms_per_step is wall time between synchronisations over --steps steps after --warmup.  The per-launch figures come from HIP events
recorded around every LVC launch (forward, backward_data, backward_weight) and around the predictor's forward and backward as a
whole, on one extra step: the sum of each kind over that step, in microseconds.

    python tools/melglow_step.py [--steps 5] [--warmup 2] [--batch 8] [--samples 22016]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=22016)
    args = ap.parse_args()

    import numpy as np
    import torch
    import fill
    import make_golden_melglow as mgg
    import constant_memory_waveglow_amd as cm
    from constant_memory_waveglow_amd import engine, melglow

    dev = torch.device("cuda:0")
    arch = mgg.ARCH_FULL
    m = cm.MelGlow(memory_efficient=True, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(m, "mg_full/", arch).items()})
    m = m.to(dev).train()
    crit = cm.WaveGlowLoss(fill.SIGMA)
    audio, h = mgg.inputs("mg_step", args.batch, args.samples, arch["n_mels"], arch["hop_size"])
    audio, h = torch.from_numpy(audio).to(dev), torch.from_numpy(h).to(dev)

    def one():
        m.zero_grad(set_to_none=True)
        z, ld = m(audio.clone(), h)
        crit(z, ld).backward()

    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps

    events = {}

    def timed(kind, fn):
        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            events.setdefault(kind, []).append((e0, e1))
            return out
        return run

    for name in ("lvc_forward", "lvc_backward_data", "lvc_backward_weight"):
        setattr(engine, name, timed(name, getattr(engine, name)))
    melglow._pred_forward = timed("predictor_forward", melglow._pred_forward)
    melglow._pred_backward = timed("predictor_backward", melglow._pred_backward)
    one()
    torch.cuda.synchronize()
    us = {k: round(sum(a.elapsed_time(b) for a, b in v) * 1e3, 1) for k, v in events.items()}
    counts = {k: len(v) for k, v in events.items()}
    print(json.dumps({
        "model": "melglow", "batch": args.batch, "samples": args.samples, "steps": args.steps,
        "ms_per_step": round(ms, 3), "samples_per_s": round(args.batch * args.samples / (ms * 1e-3), 1),
        "lvc_us": {k: us[k] for k in ("lvc_forward", "lvc_backward_data", "lvc_backward_weight")},
        "predictor_us": {k: us[k] for k in ("predictor_forward", "predictor_backward")},
        "launches": counts, "device": torch.cuda.get_device_name(dev),
    }))


if __name__ == "__main__":
    main()
