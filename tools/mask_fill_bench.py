#!/usr/bin/env python3
"""mask_fill_bench.py -- what the fill kinds of missing values cost and what they save: a 512^3 fp32 turbulence volume in
256^3 chunks with a ball of NaNs of about a third of the samples, and with NaNs where a low-frequency field exceeds a
threshold (blobs with long, curved boundaries).

Per mask and per fill kind (the midrange of the valid samples, a value of the caller's, the smooth pull-push fill):
  (a) mask_make with the fill, in ms and as bytes moved over time.  The bytes are those of the kernel table of DESIGN.md
      0h: the midrange and the value read the volume twice and write it once; the smooth fill reads it three times,
      writes it once, and writes and reads the levels of its pyramid
  (b) compress_masked at 2 bits per sample, in ms
  (c) the container's bytes in mode 3 at two tolerances (1e-3 and 1e-4 of the valid samples' range) and in mode 2 at 80 dB
  (d) the PSNR of quality_masked over the valid samples at 2 bits per sample in mode 1

The yardstick for time is the midrange fill.  With --baseline-lib PATH (another build of the library, e.g. the parent
commit's) the midrange calls -- sperrhip_mask_make_dev and sperrhip_compress_masked_dev, through ctypes alone -- are
timed on that build too, in a child process that has the device to itself, to show that the old path did not move.

Every time is the median (and min ... max) of --runs calls after --warmup, each timed with events on the current stream
around the call alone; the sides of a comparison alternate run by run.

  python tools/mask_fill_bench.py [--runs 15] [--warmup 3] [--n 512] [--baseline-lib sperr_amd/libsperr_hip_parent.so]
                                  [--out profiles/mask_fill_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_sz, _vp = C.c_size_t, C.c_void_p
BPP = 2.0
VALUE = 0.0


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def timed(torch, fns, runs, warmup):
    """{name: [ms]} of the calls in fns, alternating run by run"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return ms


def make_masks(torch, n):
    ax = torch.arange(n, device="cuda", dtype=torch.float32)
    c = ax - n / 2
    r2 = c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2
    radius = n * (1.0 / (4.0 * math.pi)) ** (1.0 / 3.0)      # 4/3 pi r^3 = n^3 / 3
    w = 2.0 * math.pi * ax / n
    z, y, x = w[:, None, None], w[None, :, None], w[None, None, :]
    low = torch.sin(1.5 * x + 0.3) * torch.cos(1.1 * y) + 0.7 * torch.sin(0.9 * z + 1.0) + 0.5 * torch.cos(x + y + z)
    return {"ball": r2 <= radius * radius, "blobs": low > 0.45}


def wire_midrange(lib):
    lib.sperrhip_mask_max_size.restype = _sz
    lib.sperrhip_mask_max_size.argtypes = [_sz]
    lib.sperrhip_max_compressed_size.restype = _sz
    lib.sperrhip_max_compressed_size.argtypes = [_sz] * 6 + [C.c_int, C.c_double]
    lib.sperrhip_mask_make_dev.restype = C.c_int
    lib.sperrhip_mask_make_dev.argtypes = [_vp, C.c_int, _sz, C.c_int, C.c_double, _vp, _vp, _sz, C.POINTER(_sz),
                                           C.POINTER(_sz), _vp]
    lib.sperrhip_compress_masked_dev.restype = C.c_int
    lib.sperrhip_compress_masked_dev.argtypes = [_vp, C.c_int] + [_sz] * 6 + [C.c_int, C.c_double, C.c_int, C.c_double,
                                                                             _vp, _sz, C.POINTER(_sz), _vp, _sz,
                                                                             C.POINTER(_sz), C.POINTER(_sz), _vp]
    return lib


def midrange_calls(torch, lib, v, chunks):
    """the two calls of the parent's interface, through ctypes alone: {name: fn} and what they leave behind"""
    n = v.shape[0]
    nsamp = v.numel()
    filled = torch.empty_like(v)
    buf = torch.empty(lib.sperrhip_mask_max_size(nsamp), dtype=torch.uint8, device="cuda")
    cap = lib.sperrhip_max_compressed_size(n, n, n, *chunks, 1, BPP)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    mlen, cnt, dlen = _sz(0), _sz(0), _sz(0)
    st = torch.cuda.current_stream().cuda_stream

    def make():
        assert lib.sperrhip_mask_make_dev(v.data_ptr(), 1, nsamp, 1, 0.0, filled.data_ptr(), buf.data_ptr(), buf.numel(),
                                          C.byref(mlen), C.byref(cnt), st) == 0

    def compress():
        assert lib.sperrhip_compress_masked_dev(v.data_ptr(), 1, n, n, n, *chunks, 1, BPP, 1, 0.0, dst.data_ptr(), cap,
                                                C.byref(dlen), buf.data_ptr(), buf.numel(), C.byref(mlen),
                                                C.byref(cnt), st) == 0
    return {"mask_make": make, "compress_masked": compress}, (mlen, dlen)


def baseline(args):
    """child process: the midrange calls on the library at args.child, which need not have the fill calls"""
    import torch
    from sperr_amd.synth import turbulence_torch
    lib = wire_midrange(C.CDLL(args.child))
    n = args.n
    chunks = (min(256, n),) * 3
    base = turbulence_torch((n, n, n), "cuda", dtype=torch.float32)
    out = {}
    for name, m in make_masks(torch, n).items():
        v = torch.where(m, torch.full_like(base, float("nan")), base)
        fns, (mlen, dlen) = midrange_calls(torch, lib, v, chunks)
        ms = timed(torch, fns, args.runs, args.warmup)
        out[name] = {"mask_make": stats(ms["mask_make"]), "compress_masked": stats(ms["compress_masked"]),
                     "mask_bytes": mlen.value, "container_bytes": dlen.value}
        del v
    print("BASELINE " + json.dumps(out), flush=True)
    return 0


def bytes_moved(n_samples, esz, mask_len, fill, shape, top_cells):
    """the passes of the kernel table: survey (read), pack (the bit array and the stream), the fill kernels"""
    words = 8 * ((n_samples + 63) // 64)
    common = esz * n_samples + words + words + mask_len                # survey reads, stores the bits; pack reads them
    if fill != "smooth":
        return common + 2 * esz * n_samples + words                   # k_mask_fill: read, write, the bits
    cells = [shape]
    while max(cells[-1]) > 1:
        cells.append(tuple((d + 1) // 2 for d in cells[-1]))
    c = [s[0] * s[1] * s[2] for s in cells]
    g = max(1, sum(1 for k in c[1:] if k > top_cells))
    moved = common + esz * n_samples + words + 8 * c[1]               # pull0: the samples, the bits, level 1
    for lev in range(1, g):
        moved += 8 * (c[lev] + c[lev + 1])                            # pull: read l, write l + 1
        moved += 8 * (c[lev + 1] + 2 * c[lev])                        # push: read l + 1, read and complete l
    moved += 8 * 2 * c[g]                                             # top: read and complete level G
    return moved + 2 * esz * n_samples + words + 8 * c[1]             # fill_smooth: read, write, the bits, level 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_fill_bench.json"))
    args = ap.parse_args()
    if args.child:
        return baseline(args)

    base_res = None
    if args.baseline_lib:   # (first: the child has the device to itself, and this build's runs follow it)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(args.baseline_lib), "--n", str(args.n),
               "--runs", str(args.runs), "--warmup", str(args.warmup)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("BASELINE ")]
        if res.returncode != 0 or not line:
            sys.stderr.write(res.stdout + res.stderr)
            return 2
        base_res = json.loads(line[-1][len("BASELINE "):])

    import torch
    from sperr_amd.api import SperrHip
    from sperr_amd.synth import turbulence_torch
    text = open(os.path.join(ROOT, "sperr_amd", "csrc", "mask_fill.h")).read()
    top_cells = int(re.search(r"constexpr\s+uint32_t\s+kMaskTopCells\s*=\s*(\d+)\s*;", text).group(1))
    eng = SperrHip()
    n = args.n
    chunks = (min(256, n),) * 3
    nsamp = n ** 3
    base = turbulence_torch((n, n, n), "cuda", dtype=torch.float32)
    nan = float("nan")
    fills = {"midrange": "midrange", "value": VALUE, "smooth": "smooth"}
    result = {"volume": [n, n, n], "dtype": "float32", "chunks": list(chunks), "bpp": BPP, "runs": args.runs,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "value_fill": VALUE,
              "kMaskTopCells": top_cells,
              "baseline_lib": os.path.basename(args.baseline_lib) if args.baseline_lib else None, "cases": {}}
    for name, m in make_masks(torch, n).items():
        v = torch.where(m, torch.full_like(base, nan), base)
        nmiss = int(m.sum())
        valid = base[~m]
        span = float(valid.max() - valid.min())
        del valid
        filled = torch.empty_like(v)
        stream, cnt = eng.mask_make(v, filled_out=filled)
        assert cnt == nmiss
        case = {"missing": nmiss, "fraction": round(nmiss / nsamp, 4), "kind": eng.mask_parse(stream)[2],
                "mask_bytes": stream.numel(), "valid_range": span, "fills": {}}
        # the parent's interface on this build, beside the parent's own figures
        fns, _ = midrange_calls(torch, eng.lib, v, chunks)
        ms = timed(torch, fns, args.runs, args.warmup)
        case["midrange_ctypes"] = {k: stats(t) for k, t in ms.items()}
        if base_res:
            case["midrange_ctypes_baseline"] = {k: base_res[name][k] for k in ("mask_make", "compress_masked")}
            assert base_res[name]["mask_bytes"] == stream.numel()
        # (a) and (b): the three fills side by side
        ms_make = timed(torch, {k: (lambda f=f: eng.mask_make(v, filled_out=filled, fill=f)) for k, f in fills.items()},
                        args.runs, args.warmup)
        ms_comp = timed(torch, {k: (lambda f=f: eng.compress_masked(v, chunks, BPP, fill=f)) for k, f in fills.items()},
                        args.runs, args.warmup)
        tols = {"pwe_1e-3_of_range": (3, 1e-3 * span), "pwe_1e-4_of_range": (3, 1e-4 * span), "psnr_80": (2, 80.0)}
        for k, f in fills.items():
            moved = bytes_moved(nsamp, 4, stream.numel(), k, (n, n, n), top_cells)
            r = {"mask_make": dict(stats(ms_make[k]), bytes_moved=moved,
                                   GBps=round(moved / statistics.median(ms_make[k]) / 1e6, 1)),
                 "compress_masked": stats(ms_comp[k]), "container_bytes": {}}
            for label, (mode, q) in tols.items():
                container, _ = eng.compress_masked(v, chunks, q, mode=mode, fill=f)
                r["container_bytes"][label] = container.numel()
            container, s2 = eng.compress_masked(v, chunks, BPP, fill=f)
            assert torch.equal(s2, stream)
            r["container_bytes"]["rate_2bpp"] = container.numel()
            back = eng.decompress_masked(container, stream, nan)
            qual = eng.quality_masked(v, back, stream)
            r["psnr_valid_2bpp"] = round(qual.psnr, 3)
            r["rmse_valid_2bpp"] = qual.rmse
            del back, container
            case["fills"][k] = r
        for label in list(tols) + ["rate_2bpp"]:
            a = case["fills"]["midrange"]["container_bytes"][label]
            case["fills"]["smooth"].setdefault("bytes_vs_midrange", {})[label] = \
                round(case["fills"]["smooth"]["container_bytes"][label] / a, 4)
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        del v, filled
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    eng.release()
    return 0


if __name__ == "__main__":
    sys.exit(main())
