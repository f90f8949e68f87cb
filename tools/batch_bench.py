#!/usr/bin/env python3
"""batch_bench.py -- a batch of same-shape volumes in one call against a loop of single-volume calls.

For each case N x edge^3 (fp32 volumes from sperr_amd/synth.py, one seed per volume, device-resident, chunks of
edge^3, i.e. one chunk per volume; --mode 2 at --quality dB by default) it times

  compress_batch    SperrHip.compress_batch on the (N, edge, edge, edge) tensor
  compress_loop     SperrHip.compress of every volume, one after the other
  decompress_batch  SperrHip.decompress_batch of the batch's containers
  decompress_loop   SperrHip.decompress of every container

each as the median of --runs runs after --warmup, wall time around a synchronised call on the current stream.  The
batch's containers must equal the loop's byte for byte and its decoded volumes the loop's bit for bit.  One JSON
document on stdout and in --out.

  python tools/batch_bench.py [--cases 4096x32,512x64,64x128,8x256] [--runs 5] [--warmup 2]
                              [--out profiles/batch_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="4096x32,512x64,64x128,8x256")
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--quality", type=float, default=80.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.json"))
    args = ap.parse_args()
    import torch

    from sperr_amd.api import SperrHip
    from sperr_amd.synth import turbulence_torch

    dev = torch.device("cuda", torch.cuda.current_device())
    eng = SperrHip()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(max(5, args.runs)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 3)

    results = []
    for case in args.cases.split(","):
        n, e = (int(x) for x in case.split("x"))
        vols = torch.empty((n, e, e, e), dtype=torch.float32, device=dev)
        for v in range(n):
            vols[v] = turbulence_torch((e, e, e), dev, seed=1000 + v)
        ch = (e, e, e)
        q, mode = args.quality, args.mode
        parts = eng.compress_batch(vols, ch, q, mode=mode)
        singles = [eng.compress(vols[v], ch, q, mode=mode).clone() for v in range(n)]
        same_c = all(torch.equal(p, s) for p, s in zip(parts, singles))
        back = eng.decompress_batch(parts)
        same_d = all(torch.equal(back[v].view(torch.int32), eng.decompress(singles[v]).view(torch.int32))
                     for v in range(n))
        out = torch.empty(eng.max_compressed_size(vols.shape[1:], ch, q, mode), dtype=torch.uint8, device=dev)
        bout = torch.empty(eng.max_compressed_size_batch(n, vols.shape[1:], ch, q, mode), dtype=torch.uint8,
                           device=dev)
        dout = torch.empty_like(vols)
        vout = torch.empty((e, e, e), dtype=torch.float32, device=dev)
        r = {"n": n, "edge": e, "mode": mode, "quality": q, "bytes_in": n * e ** 3 * 4,
             "bytes_out": sum(p.numel() for p in parts), "containers_equal": same_c, "volumes_equal": same_d}
        r["compress_batch_ms"] = timed(lambda: eng.compress_batch(vols, ch, q, mode=mode, out=bout))
        r["compress_loop_ms"] = timed(lambda: [eng.compress(vols[v], ch, q, out=out, mode=mode) for v in range(n)])
        shape = (e, e, e)
        r["decompress_batch_ms"] = timed(lambda: eng.decompress_batch(parts, out=dout))
        r["decompress_loop_ms"] = timed(lambda: [eng.decompress(s, out=vout, shape_zyx=shape) for s in singles])
        for d in ("compress", "decompress"):
            r[f"{d}_speedup"] = round(r[f"{d}_loop_ms"] / r[f"{d}_batch_ms"], 2)
            r[f"{d}_batch_GBps"] = round(r["bytes_in"] / r[f"{d}_batch_ms"] / 1e6, 2)
            r[f"{d}_loop_GBps"] = round(r["bytes_in"] / r[f"{d}_loop_ms"] / 1e6, 2)
        print(json.dumps(r), flush=True)
        results.append(r)
        del vols, parts, singles, back, dout, bout
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(dev), "runs": max(5, args.runs), "warmup": args.warmup,
           "timing": "wall ms around a synchronised call, median", "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    ok = all(r["containers_equal"] and r["volumes_equal"] for r in results)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
