"""Times MelGlow synthesis at the shipped configuration (configs/melglow_LJ_speech.json upstream: 12 flows, 48 channels, depth 7,
predictor 64 x 3) in eval() on cuda:0 and prints one JSON line.  For each of 1 x 62 frames (0.7 s), 1 x 860 frames (10 s) and 8 x 62
frames, one `infer` call (a latent drawn on the device, then the pass towards the audio) is timed between two synchronisations on

    module   the module path, launch by launch from Python (WG_MG_ENGINE=0)
    direct   the one-call engine with direct launches (wg_mg_inverse, WG_GRAPHS=0)
    graph    the one-call engine replaying its captured graph (WG_GRAPHS=1)

The three alternate call by call in one process, after --warmup rounds; min / median / max over --calls rounds each, in ms.
`launches`: for the engine, the kernel launches of one call (4 + 2 pred_layers + flows (4 + depth), the layer launches as counted by
wg_stat_mg_layer_launches); for the module path, its library calls (a call is one launch, or two for a product cut along K).

    python tools/melglow_synth.py [--calls 20] [--warmup 3]
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

MODES = {"module": {"WG_MG_ENGINE": "0", "WG_GRAPHS": "0"}, "direct": {"WG_MG_ENGINE": "1", "WG_GRAPHS": "0"},
         "graph": {"WG_MG_ENGINE": "1", "WG_GRAPHS": "1"}}
SHAPES = [(1, 62), (1, 860), (8, 62)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    import fill
    import make_golden_melglow as mgg
    import constant_memory_waveglow_amd as cm
    from constant_memory_waveglow_amd import _lib, engine

    dev = torch.device("cuda:0")
    arch = mgg.ARCH_FULL
    hop = arch["hop_size"]
    m = cm.MelGlow(memory_efficient=True, **arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mgg.param_values(m, "mg_full/", arch).items()})
    m = m.to(dev).eval()
    L = _lib.lib()

    calls = [0]
    plain_check = engine.check

    def counting_check(rc, what):
        calls[0] += 1
        return plain_check(rc, what)

    def one(mode, h):
        os.environ.update(MODES[mode])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.infer(h, sigma=0.6)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    result = {"model": "melglow", "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev), "shapes": {}}
    for B, frames in SHAPES:
        h = torch.from_numpy(fill.normal("mg_synth/mel%d" % frames, (B, arch["n_mels"], frames))).to(dev)
        for _ in range(args.warmup):
            for mode in MODES:
                _, out = one(mode, h)
                assert out.numel() == B * frames * hop and bool(torch.isfinite(out).all()), mode
        ms = {mode: [] for mode in MODES}
        for _ in range(args.calls):
            for mode in MODES:
                ms[mode].append(one(mode, h)[0])
        launches = {}
        engine.check = counting_check
        try:
            calls[0] = 0
            one("module", h)
            launches["module"] = calls[0]
        finally:
            engine.check = plain_check
        p0, l0 = L.wg_stat_mg_pass_calls(), L.wg_stat_mg_layer_launches()
        one("direct", h)
        assert L.wg_stat_mg_pass_calls() == p0 + 1
        launches["direct"] = launches["graph"] = \
            4 + 2 * arch["predict_layers"] + 4 * arch["flows"] + int(L.wg_stat_mg_layer_launches() - l0)
        entry = {}
        for mode in MODES:
            v = ms[mode]
            entry[mode] = {"ms_min": round(min(v), 3), "ms_median": round(statistics.median(v), 3), "ms_max": round(max(v), 3),
                           "launches": launches[mode], "samples_per_s": round(B * frames * hop / (statistics.median(v) * 1e-3), 1)}
        result["shapes"]["%dx%d" % (B, frames)] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
