"""Times one MRWaveGlow training step at the shipped configuration (configs/mr_waveglow_LJ_speech.json upstream: 2 levels x 4 flows and
4 prior flows, 256 channels, depth 8; batch 24 x 16 000, memory-efficient) on cuda:0 and prints one JSON line:

    {"ms_per_step": ..., "samples_per_s": ..., "mr_us": {...}, "mr_share": ..., "mr_gbps": {...}, ...}

ms_per_step is the time between two HIP events around --steps steps after --warmup (the wall time between the synchronisations is
printed next to it).  The wg_mr_* figures come from HIP events recorded around every such launch on one extra step: per entry point the
sum over that step in microseconds, the bytes those launches had to move, and the rate that makes (the kernels are streams: compare
with the 8 TB/s of the HBM); mr_share is their sum over the step's time.  An event pair around a wrapper also times the launch
latency and the host's allocation of the outputs, which dwarf a kernel of a few microseconds: these figures are UPPER BOUNDS (the line
says so in `mr_note`).  The kernels' own times come from `rocprofv3 --kernel-trace --stats -- python tools/mrwaveglow_step.py`, whose
kernel names are mr::haar_split_kernel, mr::haar_merge_kernel, mr::upsample_kernel, mr::upsample_bwd_kernel, mr::pack_kernel and
mr::unpack_kernel; divide `mr_mb` by those.  --h-grad asks for the gradient of the mel as well, which
brings the backward modes of the plumbing into the step.

    python tools/mrwaveglow_step.py [--steps 5] [--warmup 2] [--batch 24] [--samples 16000] [--h-grad]
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
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--h-grad", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import fill
    import make_golden_mrwaveglow as mrg
    import constant_memory_waveglow_amd as cm
    from constant_memory_waveglow_amd import engine

    dev = torch.device("cuda:0")
    arch = mrg.ARCH_FULL
    m = cm.MRWaveGlow(memory_efficient=True, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mrg.param_values(m, "mr_full/").items()})
    m = m.to(dev).train()
    crit = cm.WaveGlowLoss(fill.SIGMA)
    frames = -(-args.samples // arch["hop_size"])
    audio, h = mrg.inputs("mr_step", args.batch, args.samples, arch["n_mels"], frames)
    audio, h = torch.from_numpy(audio).to(dev), torch.from_numpy(h).to(dev).requires_grad_(args.h_grad)

    def one():
        m.zero_grad(set_to_none=True)
        h.grad = None
        z, ld = m(audio, h)
        crit(z, ld).backward()

    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        one()
    e1.record()
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    ms = e0.elapsed_time(e1) / args.steps

    # bytes each launch has to move (fp32): what it reads plus what it writes
    def n(t):
        return 0 if t is None else 4 * t.numel()

    traffic = {                  # (res: what the call returned; then the call's own arguments)
        "mr_haar_split": lambda res, x, mode=0, cond_rows=0: n(x) + n(res[0]) + n(res[1]) + (n(res[1]) if cond_rows else 0),
        "mr_haar_merge": lambda res, avg, diff, mode=0, channels_last=False, avg2=None: 2 * n(avg) + n(res) + (n(avg) if avg2 is not None else 0),
        "mr_upsample": lambda res, h, s, T, out=None, r0=0, head=None: n(h) + 4 * h.size(0) * h.size(1) * T + 2 * n(head),
        "mr_upsample_backward": lambda res, dout, r0, n_mels, F, s: 4 * dout.size(0) * n_mels * dout.size(2) + n(res),
        "mr_pack": lambda res, src, n_group, off, dst: 2 * n(src),
        "mr_unpack": lambda res, src, n_group, off, c: 2 * n(res),
    }
    events = {}

    def timed(kind, fn):
        def run(*a, **k):
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            res = fn(*a, **k)
            a1.record()
            events.setdefault(kind, []).append((a0, a1, traffic[kind](res, *a, **k)))
            return res
        return run

    for name in traffic:
        setattr(engine, name, timed(name, getattr(engine, name)))
    one()
    torch.cuda.synchronize()
    us = {k: round(sum(a.elapsed_time(b) for a, b, _ in v) * 1e3, 1) for k, v in events.items()}
    mb = {k: round(sum(c for _, _, c in v) / 1e6, 2) for k, v in events.items()}
    print(json.dumps({
        "model": "mr_waveglow", "batch": args.batch, "samples": args.samples, "steps": args.steps, "h_grad": args.h_grad,
        "ms_per_step": round(ms, 3), "wall_ms_per_step": round(wall_ms, 3),
        "samples_per_s": round(args.batch * args.samples / (ms * 1e-3), 1),
        "mr_us": us, "mr_mb": mb, "mr_gbps": {k: round(mb[k] * 1e6 / (us[k] * 1e-6) / 1e9, 1) for k in us if us[k] > 0},
        "mr_note": "mr_us / mr_gbps / mr_share: HIP events around the host wrappers, launch latency and allocation included (upper bounds)",
        "mr_share": round(sum(us.values()) * 1e-3 / ms, 5), "launches": {k: len(v) for k, v in events.items()},
        "device": torch.cuda.get_device_name(dev),
    }))


if __name__ == "__main__":
    main()
