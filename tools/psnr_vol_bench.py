#!/usr/bin/env python3
"""psnr_vol_bench.py -- what compression to a PSNR of the whole volume costs and what it buys, on one GPU.

  range     k_vol_range on n^3 (default 512), fp32 and fp64: the kernel alone (the library's profiler brackets the launch
            with events), its share of the HBM peak with the volume read once as the bytes, the whole value_range call
            (kernel, read-back, one wait), and torch.aminmax on the same tensor
  calls     compress_to_psnr against compress(mode=2) at --psnr dB: 256^3 in one chunk and in 64^3 chunks, 512^3 in 128^3
            and in 256^3 chunks, on sperr_amd.synth.turbulence_torch and on the Gaussian puff of tools/size_bench.py.  Mode 2
            is timed twice: on this build, alternating with compress_to_psnr run by run, and -- with --baseline-lib -- on
            the parent commit's build in a child process per case, through the C ABI alone.  Per case also the bytes and
            the PSNR of the volume of both containers, and the host waits of the q search per batch: none for the
            ladder; two plus one per rung walked for mode 2 (the rungs are counted from the chunk headers' q)
  ladder    with --merge-stats CSV: the rows of k_mse_ladder and k_mse_strides of a `rocprofv3 --kernel-trace --stats`
            run of `psnr_vol_bench.py --prof-workload` (a run of its own: 512^3 in 256^3 chunks, both calls) are added

Every time is the median (and min ... max) of --runs calls after --warmup, each timed with events on the current stream.

  python tools/psnr_vol_bench.py [--runs 15] [--warmup 3] [--psnr 80] [--baseline-lib PATH] [--out profiles/psnr_vol_bench.json]
"""
import argparse
import csv
import ctypes as C
import json
import math
import os
import statistics
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8.0e12   # bytes per second
CASES = [(256, 256), (256, 64), (512, 128), (512, 256)]


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def field(torch, name, n):
    from size_bench import plume_field
    from sperr_amd.synth import turbulence_torch
    return turbulence_torch((n, n, n), "cuda").contiguous() if name == "turbulence" else plume_field(torch, n)


def timed(torch, fns, runs, warmup):
    from size_bench import timed as t
    return t(torch, fns, runs, warmup)


def child(args):
    """child process: mode 2 of another build, through its C ABI alone"""
    import torch
    lib = C.CDLL(args.child)
    sz, vp = C.c_size_t, C.c_void_p
    lib.sperrhip_max_compressed_size.restype = sz
    lib.sperrhip_max_compressed_size.argtypes = [sz] * 6 + [C.c_int, C.c_double]
    lib.sperrhip_compress_dev.restype = C.c_int
    lib.sperrhip_compress_dev.argtypes = [vp, C.c_int] + [sz] * 6 + [C.c_int, C.c_double, vp, sz, C.POINTER(sz), vp]
    n, ch = args.size, args.chunk
    vol = field(torch, args.field, n)
    out = torch.empty(lib.sperrhip_max_compressed_size(n, n, n, ch, ch, ch, 2, args.psnr), dtype=torch.uint8, device="cuda")
    ln = sz(0)

    def call():
        rtn = lib.sperrhip_compress_dev(vol.data_ptr(), 1, n, n, n, ch, ch, ch, 2, args.psnr, out.data_ptr(), out.numel(),
                                        C.byref(ln), vp(torch.cuda.current_stream().cuda_stream))
        assert rtn == 0, rtn
    ms = timed(torch, {"mode2": call}, args.runs, args.warmup)
    print("BASELINE " + json.dumps({"mode2": stats(ms["mode2"]), "bytes": ln.value}), flush=True)


def psnr_of(torch, eng, vol, container):
    back = eng.decompress(container, output_float=True)
    d = back.to(torch.float64) - vol.to(torch.float64)
    rng = float(vol.max().double() - vol.min().double())
    return 10.0 * math.log10(rng * rng / float((d * d).mean()))


def mode2_rungs(torch, vol, chunks, container, psnr):
    """the rungs mode 2's search walked, chunk by chunk, from the chunk headers' q: q = q_0 / 2^(k/4) with q_0 from the
    chunk's own range"""
    from sperr_amd.farm import chunk_grid, split_container
    _, _, _, parts = split_container(bytes(container.cpu().numpy()))
    rungs = []
    for (x0, lx, y0, ly, z0, lz), part in zip(chunk_grid(tuple(vol.shape), chunks), parts):
        if part[0] & 1:
            continue
        ck = vol[z0:z0 + lz, y0:y0 + ly, x0:x0 + lx].double()
        rng = float(ck.max() - ck.min())
        q0 = 2.0 * math.sqrt(3.0 * rng * rng * 10.0 ** (-psnr / 10.0))
        rungs.append(int(round(4.0 * math.log2(q0 / struct.unpack_from("<d", part, 9)[0]))))
    return rungs


def prof_workload(args):
    import torch
    from sperr_amd.api import SperrHip
    eng = SperrHip()
    vol = field(torch, "turbulence", 512)
    for _ in range(5):
        eng.compress_to_psnr(vol, (256,) * 3, args.psnr)
        eng.compress(vol, (256,) * 3, args.psnr, mode=2)
    torch.cuda.synchronize()


def merge_stats(args):
    rec = json.load(open(args.out))
    rows = {}
    for row in csv.DictReader(open(args.merge_stats)):
        name = row.get("Name", "")
        for k in ("k_mse_ladder_pick", "k_mse_ladder", "k_mse_strides", "k_mse_final"):
            if name.startswith("sperrhip::" + k + "(") or name.startswith(k + "(") or name == k or name == "sperrhip::" + k:
                rows[k] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                           "max_ns": float(row["MaxNs"])}
    rec["ladder_kernels_rocprofv3"] = rows
    if "k_mse_ladder" in rows and "k_mse_strides" in rows:
        rec["ladder_kernels_rocprofv3"]["five_rungs_over_one"] = round(rows["k_mse_ladder"]["average_ns"] /
                                                                       rows["k_mse_strides"]["average_ns"], 3)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["ladder_kernels_rocprofv3"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--psnr", type=float, default=80.0)
    ap.add_argument("--range-size", type=int, default=512)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psnr_vol_bench.json"))
    ap.add_argument("--prof-workload", action="store_true")
    ap.add_argument("--merge-stats", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--size", type=int, default=256, help=argparse.SUPPRESS)
    ap.add_argument("--chunk", type=int, default=256, help=argparse.SUPPRESS)
    ap.add_argument("--field", default="turbulence", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.prof_workload:
        return prof_workload(args)
    if args.merge_stats:
        return merge_stats(args)
    import torch
    from sperr_amd.api import SperrHip
    from size_bench import kernel_ms
    eng = SperrHip()
    rec = {"runs": args.runs, "warmup": args.warmup, "psnr": args.psnr, "device": torch.cuda.get_device_name(0),
           "baseline_lib": os.path.basename(args.baseline_lib) if args.baseline_lib else None, "range": {}, "calls": {}}
    n = args.range_size
    for dt in (torch.float32, torch.float64):
        vol = field(torch, "turbulence", n).to(dt)
        ms = timed(torch, {"value_range": lambda: eng.value_range(vol), "torch_aminmax": lambda: torch.aminmax(vol)},
                   args.runs, args.warmup)
        k = kernel_ms(torch, eng, lambda: eng.value_range(vol), "k_vol_range", args.runs, 1)
        nbytes = vol.numel() * vol.element_size()
        lo, hi = eng.value_range(vol)
        mn, mx = torch.aminmax(vol)
        assert (lo, hi) == (float(mn), float(mx))
        r = {"bytes": nbytes, "k_vol_range": stats(k), "value_range_call": stats(ms["value_range"]),
             "torch_aminmax": stats(ms["torch_aminmax"]),
             "k_vol_range_fraction_of_hbm_peak": round(nbytes / (statistics.median(k) * 1e-3) / HBM_PEAK, 4),
             "torch_aminmax_fraction_of_hbm_peak": round(nbytes / (statistics.median(ms["torch_aminmax"]) * 1e-3) / HBM_PEAK, 4)}
        rec["range"]["%d^3 %s" % (n, str(dt).split(".")[-1])] = r
        print(n, dt, json.dumps(r), flush=True)
        del vol
    for name in ("turbulence", "plume"):
        for size, ch in CASES:
            case = "%s %d^3 in %d^3" % (name, size, ch)
            r = {}
            if args.baseline_lib:   # (first: the child has the device to itself, and this build's runs follow it)
                cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child",
                       os.path.abspath(args.baseline_lib), "--size", str(size), "--chunk", str(ch), "--field", name,
                       "--psnr", str(args.psnr), "--runs", str(args.runs), "--warmup", str(args.warmup)]
                res = subprocess.run(cmd, capture_output=True, text=True)
                line = [ln for ln in res.stdout.split("\n") if ln.startswith("BASELINE ")]
                if res.returncode != 0 or not line:   # (nothing more is started on the device after a child that failed)
                    print(res.stdout[-2000:] + res.stderr[-3000:], file=sys.stderr)
                    sys.exit(1)
                r["parent_build"] = json.loads(line[-1][len("BASELINE "):])
            vol = field(torch, name, size)
            chunks = (ch, ch, ch)
            out = torch.empty(eng.max_compressed_size(vol.shape, chunks, args.psnr, 2), dtype=torch.uint8, device="cuda")
            ms = timed(torch, {"compress_to_psnr": lambda: eng.compress_to_psnr(vol, chunks, args.psnr, out=out),
                               "mode2": lambda: eng.compress(vol, chunks, args.psnr, out=out, mode=2)}, args.runs, args.warmup)
            r.update({k: stats(v) for k, v in ms.items()})
            base = r["parent_build"]["mode2"]["median"] if "parent_build" in r else r["mode2"]["median"]
            r["ratio_to_mode2"] = round(r["compress_to_psnr"]["median"] / base, 3)
            a = eng.compress_to_psnr(vol, chunks, args.psnr).clone()
            b = eng.compress(vol, chunks, args.psnr, mode=2).clone()
            if "parent_build" in r:
                assert r["parent_build"]["bytes"] == b.numel()
            rungs = mode2_rungs(torch, vol, chunks, b, args.psnr)
            r.update({"bytes": a.numel(), "mode2_bytes": b.numel(), "psnr_db": round(psnr_of(torch, eng, vol, a), 2),
                      "mode2_psnr_db": round(psnr_of(torch, eng, vol, b), 2), "q_search_host_waits_per_batch": 0,
                      "mode2_q_search_host_waits_per_batch": 2 + (max(rungs) + 1 if rungs else 0),
                      "mode2_rungs_walked": [min(rungs), max(rungs)] if rungs else None})
            rec["calls"][case] = r
            print(case, json.dumps(r), flush=True)
            del vol, out
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
