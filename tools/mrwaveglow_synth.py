"""Times MRWaveGlow synthesis at the shipped configuration (configs/mr_waveglow_LJ_speech.json upstream: 3 levels of 4 flows, 4 prior
flows, 256 channels, depth 8) in eval() on cuda:0 and prints one JSON line per shape.  For each of 1 x 62 frames (0.7 s), 1 x 860
frames (10 s) and 8 x 62 frames, one `infer` call (a latent drawn on the device, then the pass towards the audio) is timed between
two synchronisations on

    module   the module path, block by block from Python (WG_MR_ENGINE=0)
    direct   the one-call engine with direct launches (wg_mr_inverse, WG_GRAPHS=0)
    graph    the one-call engine replaying its captured graph (WG_GRAPHS=1)

The three alternate call by call in one process, after --warmup rounds; min / median / max over --calls rounds each, in ms.
Launches per call are not counted here (wg_timer_* records the timed kernel classes only): they come from a kernel trace of one path,
as in the second command below (`Calls` of the stats file over the number of calls, the one-off weight pack apart).
For orientation the same three shapes through WaveGlow's wg_inverse (the shipped 12-flow configuration, direct and replayed) in the
same process: `waveglow` in each line.  --out appends the lines to a file (profiles/mr_synth.jsonl).  --shape, --only and --no-waveglow
narrow the run to what a profiler should see, e.g. the engine's direct launches of the 0.7 s call alone:

    python tools/mrwaveglow_synth.py [--calls 20] [--warmup 3] [--out profiles/mr_synth.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/mrwaveglow_synth.py --shape 1x62 --only direct --no-waveglow --calls 10 --warmup 2
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

MODES = {"module": {"WG_MR_ENGINE": "0", "WG_GRAPHS": "0"}, "direct": {"WG_MR_ENGINE": "1", "WG_GRAPHS": "0"},
         "graph": {"WG_MR_ENGINE": "1", "WG_GRAPHS": "1"}}
WG_MODES = {"direct": {"WG_GRAPHS": "0"}, "graph": {"WG_GRAPHS": "1"}}
SHAPES = [(1, 62), (1, 860), (8, 62)]


def summary(v):
    return {"ms_min": round(min(v), 3), "ms_median": round(statistics.median(v), 3), "ms_max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="BxFRAMES: this shape alone")
    ap.add_argument("--only", default=None, choices=list(MODES), help="this path alone")
    ap.add_argument("--no-waveglow", action="store_true")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in args.shape.split("x"))] if args.shape else SHAPES
    modes = {args.only: MODES[args.only]} if args.only else MODES

    import numpy as np
    import torch
    import fill
    import make_golden_mrwaveglow as mrg
    import constant_memory_waveglow_amd as cm
    from constant_memory_waveglow_amd import _lib

    dev = torch.device("cuda:0")
    arch = mrg.ARCH_FULL
    hop = arch["hop_size"]
    m = cm.MRWaveGlow(memory_efficient=True, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mrg.param_values(m, "mr_full/").items()})
    m = m.to(dev).eval()
    wg = None
    if not args.no_waveglow:
        cfg = fill.CONFIGS["c2"]
        wg = cm.WaveGlow(memory_efficient=True, bias=False, **cfg)
        wg.load_state_dict({k: torch.from_numpy(v) for k, v in fill.fill_params(fill.model_param_specs(cfg), "c2/").items()})
        wg = wg.to(dev).eval()
    L = _lib.lib()

    def one(model, env, h):
        os.environ.update(env)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.infer(h, sigma=0.6)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for B, frames in shapes:
        h = torch.from_numpy(fill.normal("mr_synth/mel%d" % frames, (B, arch["n_mels"], frames))).to(dev)
        runs = [("mr", mode, m, env) for mode, env in modes.items()]
        if wg is not None:
            runs += [("wg", mode, wg, env) for mode, env in WG_MODES.items()]
        for _ in range(args.warmup):
            for _, mode, model, env in runs:
                _, out = one(model, env, h)
                assert out.numel() == B * frames * hop and bool(torch.isfinite(out).all()), mode
        ms = {(which, mode): [] for which, mode, _, _ in runs}
        for _ in range(args.calls):
            for which, mode, model, env in runs:
                ms[which, mode].append(one(model, env, h)[0])
        for mode, env in modes.items():                      # each path is the one its name says
            p0 = L.wg_stat_mr_pass_calls()
            one(m, env, h)
            assert L.wg_stat_mr_pass_calls() - p0 == (mode != "module"), mode
        line = {"model": "mrwaveglow", "shape": "%dx%d" % (B, frames), "calls": args.calls, "warmup": args.warmup,
                "device": torch.cuda.get_device_name(dev), "precision": os.environ.get("WG_PRECISION", "bf16x3p")}
        for mode in modes:
            v = ms["mr", mode]
            line[mode] = dict(summary(v), samples_per_s=round(B * frames * hop / (statistics.median(v) * 1e-3), 1))
        if wg is not None:
            line["waveglow"] = {mode: summary(ms["wg", mode]) for mode in WG_MODES}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
