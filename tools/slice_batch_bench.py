#!/usr/bin/env python3
"""slice_batch_bench.py -- a batch of same-shape 2D slices in one call against a loop of single-slice calls.

For each case N x (y x x) (fp32 slices from sperr_amd/synth.py, one seed per slice, device-resident; --mode 2 at
--quality dB by default) it times

  compress_batch    SperrHip.compress_2d_batch on the (N, y, x) tensor
  compress_loop     sperrhip_compress_2d_dev of every slice, one after the other, into one buffer
  decompress_batch  SperrHip.decompress_2d_batch of the batch's streams
  decompress_loop   sperrhip_decompress_2d_dev of every stream, into one buffer

each over --runs runs (at least 5) after --warmup, wall time around a synchronised call on the current stream: min,
median and max are recorded, the median is the figure.  The batch's streams must equal the loop's byte for byte and
its decoded slices the loop's bit for bit.  With --baseline-lib PATH (another build of the library, e.g. the parent
commit's, which need not have the batch calls) the same two loops are also timed on that build, in a child process
of its own per case, so that the two builds' runs alternate case by case.  One JSON document on stdout and in --out.

  python tools/slice_batch_bench.py [--cases 64x999x999,256x256x256,1024x96x121,8x999x999] [--runs 5] [--warmup 2]
                                    [--baseline-lib sperr_amd/libsperr_hip_parent.so]
                                    [--out profiles/slice_batch_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_sz = C.c_size_t


def make_slices(torch, dev, n, dy, dx):
    from sperr_amd.synth import turbulence_torch
    imgs = torch.empty((n, dy, dx), dtype=torch.float32, device=dev)
    for s in range(n):
        imgs[s] = turbulence_torch((1, dy, dx), dev, seed=1000 + s)[0]
    return imgs


def timed(torch, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(max(5, runs)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def launches(torch, eng, fn):
    torch.cuda.synchronize()
    eng.profile(True)
    fn()
    torch.cuda.synchronize()
    rep = eng.profile_report()
    eng.profile(False)
    return sum(n for _, n in rep.values())


def wire(lib):
    lib.sperrhip_max_compressed_size_2d.restype = _sz
    lib.sperrhip_max_compressed_size_2d.argtypes = [_sz, _sz, C.c_int, C.c_double]
    lib.sperrhip_compress_2d_dev.argtypes = [C.c_void_p, C.c_int, _sz, _sz, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                             _sz, C.POINTER(_sz), C.c_void_p]
    lib.sperrhip_decompress_2d_dev.argtypes = [C.c_void_p, _sz, C.c_int, _sz, _sz, C.c_void_p, _sz, C.c_void_p]
    return lib


def single_loops(torch, lib, imgs, args):
    """the two loops of single-slice calls through the C ABI of `lib` (this build's or another's), into buffers
    allocated once: what the batch calls are measured against"""
    n, dy, dx = imgs.shape
    cap = lib.sperrhip_max_compressed_size_2d(dx, dy, args.mode, args.quality)
    out = torch.empty(cap, dtype=torch.uint8, device=imgs.device)
    vout = torch.empty((dy, dx), dtype=torch.float32, device=imgs.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def comp(s, dst):
        ln = _sz(0)
        rc = lib.sperrhip_compress_2d_dev(imgs[s].data_ptr(), 1, dx, dy, args.mode, args.quality, 0, dst.data_ptr(),
                                          dst.numel(), C.byref(ln), stream)
        assert rc == 0
        return dst[:ln.value]

    def decomp(t):
        rc = lib.sperrhip_decompress_2d_dev(t.data_ptr(), t.numel(), 1, dx, dy, vout.data_ptr(), vout.numel() * 4,
                                            stream)
        assert rc == 0

    singles = [comp(s, out).clone() for s in range(n)]
    return {"compress_loop_ms": timed(torch, lambda: [comp(s, out) for s in range(n)], args.runs, args.warmup),
            "decompress_loop_ms": timed(torch, lambda: [decomp(t) for t in singles], args.runs, args.warmup),
            "bytes_out": sum(t.numel() for t in singles)}


def baseline_loops(args):
    """child process: the loops on the library at args.child_loop, which need not have the batch calls"""
    import torch
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    lib = wire(C.CDLL(args.child_loop))
    dev = torch.device("cuda", torch.cuda.current_device())
    n, dy, dx = (int(x) for x in args.cases.split("x"))
    r = single_loops(torch, lib, make_slices(torch, dev, n, dy, dx), args)
    print("BASELINE " + json.dumps(r), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64x999x999,256x256x256,1024x96x121,8x999x999")
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--quality", type=float, default=90.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child-loop", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slice_batch_bench.json"))
    args = ap.parse_args()
    if args.child_loop:
        return baseline_loops(args)
    import torch

    from sperr_amd.api import SperrHip

    dev = torch.device("cuda", torch.cuda.current_device())
    eng = SperrHip()
    q, mode = args.quality, args.mode
    results = []
    for case in args.cases.split(","):
        n, dy, dx = (int(x) for x in case.split("x"))
        shape = (dy, dx)
        r = {"n": n, "shape_yx": [dy, dx], "mode": mode, "quality": q, "bytes_in": n * dy * dx * 4}
        if args.baseline_lib:   # (first: the child has the device to itself, and this build's runs follow it)
            cmd = [sys.executable, os.path.abspath(__file__), "--child-loop", os.path.abspath(args.baseline_lib),
                   "--cases", case, "--mode", str(mode), "--quality", str(q), "--runs", str(args.runs), "--warmup",
                   str(args.warmup)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("BASELINE ")]
            if res.returncode != 0 or not line:
                sys.stderr.write(res.stdout + res.stderr)
                return 2
            r["baseline"] = json.loads(line[-1][len("BASELINE "):])
        imgs = make_slices(torch, dev, n, dy, dx)
        parts = eng.compress_2d_batch(imgs, q, mode=mode)
        singles = [eng.compress_2d(imgs[s], q, mode=mode).clone() for s in range(n)]
        r["bytes_out"] = sum(p.numel() for p in parts)
        r["streams_equal"] = all(torch.equal(p, s) for p, s in zip(parts, singles))
        back = eng.decompress_2d_batch(parts, shape)
        r["slices_equal"] = all(torch.equal(back[s].view(torch.int32),
                                            eng.decompress_2d(singles[s], shape).view(torch.int32)) for s in range(n))
        if "baseline" in r:
            r["baseline_bytes_equal"] = r["baseline"]["bytes_out"] == r["bytes_out"]
        bout = torch.empty(eng.max_compressed_size_2d_batch(n, shape, q, mode), dtype=torch.uint8, device=dev)
        dout = torch.empty_like(imgs)
        r["compress_batch_ms"] = timed(torch, lambda: eng.compress_2d_batch(imgs, q, mode=mode, out=bout), args.runs,
                                       args.warmup)
        r["decompress_batch_ms"] = timed(torch, lambda: eng.decompress_2d_batch(parts, shape, out=dout), args.runs,
                                         args.warmup)
        loops = single_loops(torch, wire(eng.lib), imgs, args)
        r["compress_loop_ms"], r["decompress_loop_ms"] = loops["compress_loop_ms"], loops["decompress_loop_ms"]
        k = min(n, 8)   # (launch counts: the batch, and a loop over the first slices scaled to n)
        r["launches"] = {
            "compress_batch": launches(torch, eng, lambda: eng.compress_2d_batch(imgs, q, mode=mode, out=bout)),
            "compress_loop": launches(torch, eng, lambda: [eng.compress_2d(imgs[s], q, mode=mode)
                                                            for s in range(k)]) * n // k,
            "decompress_batch": launches(torch, eng, lambda: eng.decompress_2d_batch(parts, shape, out=dout)),
            "decompress_loop": launches(torch, eng, lambda: [eng.decompress_2d(s, shape)
                                                              for s in singles[:k]]) * n // k}
        for d in ("compress", "decompress"):
            b, lp = r[f"{d}_batch_ms"], r[f"{d}_loop_ms"]
            r[f"{d}_speedup"] = round(lp["median"] / b["median"], 2)
            r[f"{d}_batch_GBps"] = round(r["bytes_in"] / b["median"] / 1e6, 2)
            r[f"{d}_loop_GBps"] = round(r["bytes_in"] / lp["median"] / 1e6, 2)
            # the batch beats the loop by more than the spread of the runs: its slowest run against the loop's fastest
            r[f"{d}_batch_beats_loop"] = b["max"] < lp["min"]
            if "baseline" in r:
                bl = r["baseline"][f"{d}_loop_ms"]
                r[f"{d}_speedup_vs_baseline"] = round(bl["median"] / b["median"], 2)
                r[f"{d}_batch_beats_baseline_loop"] = b["max"] < bl["min"]
        print(json.dumps(r), flush=True)
        results.append(r)
        del imgs, parts, singles, back, dout, bout
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(dev), "runs": max(5, args.runs), "warmup": args.warmup,
           "timing": "wall ms around a synchronised call: min / median / max of the runs",
           "baseline_lib": os.path.basename(args.baseline_lib) if args.baseline_lib else None, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    ok = all(r["streams_equal"] and r["slices_equal"] for r in results)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
