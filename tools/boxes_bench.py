#!/usr/bin/env python3
"""boxes_bench.py -- one decompress_boxes call against the loop of decompress_box calls it replaces.

Synthetic 512^3 fp32 volumes (sperr_amd/synth.py, one seed per container) in 256^3 chunks at 2 bits per sample, all
device-resident, every container a tensor of its own.  Each case warms both contenders, then times them ALTERNATELY --
one call, the loop, one call, the loop ... -- with HIP events around each on the current stream (both end with the
stream drained), --runs times; it records each contender's median, quartiles, minimum and maximum.  `spread` is the
full range of a contender's times, maximum minus minimum; `won` says whether the one call's median lies below the
loop's by more than the larger of the two spreads.

  series_N{8,32}_aligned   the chunk-aligned box 256^3 at (256, 256, 256) of every container: one chunk each
  series_N{8,32}_mid       128^3 at (192, 192, 192) of every container: eight chunks each, an eighth of a box from each
  crops                    32 crops of 64^3 at seeded origins out of 4 containers: the call stages; with the plan's
                           slot and pair counts and k_boxes_copy's time (from the profile, a run of its own) as a share
                           of the call's median

  python tools/boxes_bench.py [--size 512] [--runs 15] [--warmup 3] [--out profiles/boxes_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--bpp", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from sperr_amd.api import SperrHip
    from sperr_amd.synth import turbulence_torch

    S, C = args.size, args.chunk
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = SperrHip()
    ncont = max(args.series + [4])
    containers = []
    for i in range(ncont):
        vol = turbulence_torch((S, S, S), dev, seed=42 + i)
        containers.append(eng.compress(vol, (C, C, C), args.bpp).clone())
        del vol

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def figures(ms):
        q = statistics.quantiles(ms, n=4)
        return {"median_ms": round(statistics.median(ms), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3),
                "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "spread_ms": round(max(ms) - min(ms), 3)}

    def contest(conts, which, los, dims):
        """the one call and the loop over the same entries, alternately"""
        nbox = len(los)
        out = torch.empty((nbox, dims[2], dims[1], dims[0]), dtype=torch.float32, device=dev)
        wh = list(range(len(conts))) if which is None else which

        def one_call():
            eng.decompress_boxes(conts, los if which is not None else los[0], dims, which=which, out=out)

        def loop():
            for e in range(nbox):
                eng.decompress_box(conts[wh[e]], los[e], dims, out=out[e])

        for _ in range(args.warmup):
            one_call()
            loop()
        a, b = [], []
        for _ in range(args.runs):
            a.append(once(one_call))
            b.append(once(loop))
        fa, fb = figures(a), figures(b)
        gap = fb["median_ms"] - fa["median_ms"]
        return one_call, {"entries": nbox, "box": list(dims), "one_call": fa, "loop": fb,
                          "loop_over_one_call": round(fb["median_ms"] / fa["median_ms"], 3),
                          "won": bool(gap > max(fa["spread_ms"], fb["spread_ms"])),
                          "won_by_interquartile_range": bool(gap > max(fa["q3_ms"] - fa["q1_ms"],
                                                                        fb["q3_ms"] - fb["q1_ms"]))}

    cases = {}
    for n in args.series:
        _, cases[f"series_N{n}_aligned"] = contest(containers[:n], None, [(C, C, C)] * n, (C, C, C))
        h = C // 2
        lo = (C - h // 2,) * 3
        _, cases[f"series_N{n}_mid"] = contest(containers[:n], None, [lo] * n, (h, h, h))
    rng = np.random.default_rng(20261020)
    cd = C // 4
    which = [int(rng.integers(0, 4)) for _ in range(args.crops)]
    los = [tuple(int(rng.integers(0, S - cd + 1)) for _ in range(3)) for _ in which]
    plan = eng.boxes_plan((S, S, S), [(C, C, C)] * 4, los, (cd, cd, cd), which=which)
    one_call, crops = contest(containers[:4], which, los, (cd, cd, cd))
    eng.profile(True)
    one_call()
    copy_ms = sum(ms for name, (ms, _) in eng.profile_report().items() if "k_boxes_copy" in name)
    eng.profile(False)
    crops.update({"slots": plan["slots"], "pairs": plan["pairs"], "staged": plan["staged"],
                  "k_boxes_copy_ms": round(copy_ms, 4),
                  "k_boxes_copy_share": round(copy_ms / crops["one_call"]["median_ms"], 5)})
    cases["crops"] = crops
    line = {"metric": "boxes_decode_ms", "volume": [S, S, S], "chunks": [C, C, C], "bpp": args.bpp, "runs": args.runs,
            "warmup": args.warmup, "clock": "HIP events around each contender, alternating", "cases": cases,
            "device": torch.cuda.get_device_name(dev)}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
