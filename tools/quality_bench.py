#!/usr/bin/env python3
"""quality_bench.py -- what the quality figures of a reconstruction cost when both arrays are on the device.

Cases: 1024^3 and 512^3 in fp32 and fp64 (SperrHip.quality), and batches of 4096 x 32^3 and 64 x 128^3 fp32
(SperrHip.quality_batch).  Every call is timed with HIP events around it on the current stream -- the call ends in its
own host wait --, median and min ... max of --runs runs after --warmup.  Two yardsticks, timed alternately with the
call, run by run, in this one process:

  abi      the C entry point alone (sperrhip_quality_batch_dev), without the Python records around it
  copy     a torch device-to-device copy of as many bytes as the call's two inputs: the rate at which the data could
           stream (a copy reads AND writes that many bytes; GB/s below count the bytes read only, as for the call)
  torch    the composition a user writes without this call: max |a - b|, mean (a - b)^2, min a, max a and
           var / mean of a, fetched with one host copy.  It materialises a - b and does not give the reference's bits.

GB/s are input bytes (2 x n x sizeof T) / time; the call reads a a second time for the variance, which is not counted.
The kernels' own times come from the library's profiler in runs of their own.  One JSON line on stdout, and --out.

  python tools/quality_bench.py [--runs 15] [--warmup 3] [--out profiles/quality_bench.json] [--small]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64^3 cases only: a rehearsal of the script")
    args = ap.parse_args()

    import torch
    from sperr_amd.api import SperrHip
    eng = SperrHip()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def torch_five(a, b):
        d = a - b
        var, mean = torch.var_mean(a, unbiased=False)
        return torch.stack([d.abs().max(), (d * d).mean(), a.min(), a.max(), var, mean]).cpu()

    if args.small:
        cases = [("64^3", torch.float32, 1, 64 ** 3), ("8 x 32^3", torch.float32, 8, 32 ** 3)]
    else:
        cases = [("1024^3", torch.float32, 1, 1024 ** 3), ("1024^3", torch.float64, 1, 1024 ** 3),
                 ("512^3", torch.float32, 1, 512 ** 3), ("512^3", torch.float64, 1, 512 ** 3),
                 ("4096 x 32^3", torch.float32, 4096, 32 ** 3), ("64 x 128^3", torch.float32, 64, 128 ** 3)]
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
           "timing": "HIP events around the call, ms", "cases": []}
    for label, dt, nvol, n in cases:
        g = torch.Generator(device="cuda").manual_seed(7)
        a = torch.randn((nvol, n), dtype=dt, device="cuda", generator=g)
        b = a + 1e-3 * torch.randn((nvol, n), dtype=dt, device="cuda", generator=g)
        src, dst = torch.empty(2 * a.numel(), dtype=dt, device="cuda"), torch.empty(2 * a.numel(), dtype=dt, device="cuda")
        src.zero_()
        call = (lambda: eng.quality(a, b)) if nvol == 1 else (lambda: eng.quality_batch(a, b))
        figs = (C.c_double * (8 * nvol))()
        abi = lambda: eng.lib.sperrhip_quality_batch_dev(a.data_ptr(), b.data_ptr(), int(dt == torch.float32), nvol, n,
                                                         figs, eng._stream())   # noqa: E731
        fns = {"call": call, "abi": abi, "copy": lambda: dst.copy_(src), "torch": lambda: torch_five(a, b)}
        ms = {k: [] for k in fns}
        for it in range(args.warmup + args.runs):
            for k, fn in fns.items():
                t = timed(fn)
                if it >= args.warmup:
                    ms[k].append(t)
        eng.profile(True)
        for _ in range(3):
            call()
        kern = {k: round(v[0] / v[1], 4) for k, v in eng.profile_report().items()}
        eng.profile(False)
        nbytes = 2 * a.numel() * a.element_size()
        rec = {"case": label, "dtype": str(dt).split(".")[-1], "nvol": nvol, "n": n, "input_bytes": nbytes}
        for k in fns:
            rec[k + "_ms"] = stats(ms[k])
            rec[k + "_GBps"] = round(nbytes / statistics.median(ms[k]) / 1e6, 1)
        rec["call_over_copy"] = round(statistics.median(ms["call"]) / statistics.median(ms["copy"]), 3)
        rec["torch_over_call"] = round(statistics.median(ms["torch"]) / statistics.median(ms["call"]), 3)
        rec["kernel_ms_per_launch"] = kern
        q = call()
        q = q if nvol == 1 else q[0]
        rec["psnr"], rec["rmse"] = q.psnr, q.rmse
        out["cases"].append(rec)
        del a, b, src, dst
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
