#!/usr/bin/env python3
"""box_bench.py -- device time of sub-box decodes (sperrhip_decompress_box_dev) against the whole decode.

The bench volume (1024^3 fp32 from sperr_amd/synth.py, 256^3 chunks, 2 bits per sample), device-resident.
Every case is timed with HIP events around the call on the current stream, as the median of --runs runs
after --warmup; one JSON line on stdout (and in --out when given):

  full            sperrhip_decompress_dev, the whole volume
  box_whole       the box that is the whole volume (goes through the whole-volume decode)
  box_512_origin  512^3 at (0, 0, 0): eight chunks, nothing of them cropped
  box_256_mid     256^3 at (128, 128, 128): the same eight chunks, each cropped to an eighth
  box_256_chunk   256^3 at (256, 256, 256): exactly one chunk

  python tools/box_bench.py [--size 1024] [--runs 15] [--warmup 3] [--out profiles/box_bench.json]
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
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--bpp", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from sperr_amd.api import SperrHip
    from sperr_amd.synth import turbulence_torch

    S, C = args.size, args.chunk
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = SperrHip()
    vol = turbulence_torch((S, S, S), dev, seed=42)
    container = eng.compress(vol, (C, C, C), args.bpp).clone()
    del vol
    out = torch.empty(S * S * S, dtype=torch.float32, device=dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return round(statistics.median(ms), 3)

    def box(lo, dims):
        n = dims[0] * dims[1] * dims[2]
        return lambda: eng.decompress_box(container, lo, dims, out=out[:n].view(dims[2], dims[1], dims[0]))

    h = C // 2
    res = {
        "full": timed(lambda: eng.decompress(container, True, out=out.view(S, S, S))),
        "box_whole": timed(box((0, 0, 0), (S, S, S))),
        "box_512_origin": timed(box((0, 0, 0), (2 * C, 2 * C, 2 * C))),
        "box_256_mid": timed(box((h, h, h), (C, C, C))),
        "box_256_chunk": timed(box((C, C, C), (C, C, C))),
    }
    line = {"metric": "box_decode_ms", "volume": [S, S, S], "chunks": [C, C, C], "bpp": args.bpp,
            "runs": args.runs, "median_ms": res,
            "ratios": {"box_whole/full": round(res["box_whole"] / res["full"], 4),
                       "box_256_mid/box_512_origin": round(res["box_256_mid"] / res["box_512_origin"], 4),
                       "box_256_chunk/full": round(res["box_256_chunk"] / res["full"], 4)},
            "device": torch.cuda.get_device_name(dev)}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
