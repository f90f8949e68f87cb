#!/usr/bin/env python3
"""level_bench.py -- device time of decoding one level of the hierarchy (sperrhip_decompress_level_dev) against
the plain and the multires decode of another build of the library, e.g. the parent commit's.

The bench volume (1024^3 fp32 from sperr_amd/synth.py, 256^3 chunks), device-resident, in two cases: fixed rate at
--bpp bits per value, and point-wise error at --pwe-rel of the volume's range.  Per case, HIP events around the call
on the current stream, --runs runs after --warmup; min, median and max are kept, the median is the figure:

  level[h]        the whole level h, for every level (float output)
  level_box[h]    level h, the chunk-aligned box of a single chunk: the corner of chunk (1, 1, 1)
  box_256_chunk   sperrhip_decompress_box_dev of exactly one chunk, this build
  baseline        with --baseline-lib PATH, in a child process of its own per case (so that the two builds' runs
                  alternate case by case, and the other build need not have the level calls): full
                  (sperrhip_decompress_dev), multires (sperrhip_decompress_multires_dev) and box_256_chunk

Conditions recorded per case: every level's slowest run is not slower than the baseline's fastest plain decode, and
every one-chunk level box's slowest run is not slower than the baseline's fastest one-chunk box decode.  The
baseline's container must equal this build's byte for byte.  One JSON document on stdout and in --out.

  python tools/level_bench.py [--size 1024] [--runs 15] [--warmup 3] [--baseline-lib sperr_amd/libsperr_hip_parent.so]
                              [--out profiles/level_bench.json]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_sz, _vp = C.c_size_t, C.c_void_p


def timed(torch, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def make_volume(torch, dev, size):
    from sperr_amd.synth import turbulence_torch
    return turbulence_torch((size, size, size), dev, seed=42)


def quality_of(torch, vol, case, args):
    if case == "fixed_rate":
        return 1, args.bpp
    return 3, args.pwe_rel * float((vol.max() - vol.min()).item())


def wire(lib):
    lib.sperrhip_max_compressed_size.restype = _sz
    lib.sperrhip_max_compressed_size.argtypes = [_sz] * 6 + [C.c_int, C.c_double]
    lib.sperrhip_compress_dev.argtypes = [_vp, C.c_int, _sz, _sz, _sz, _sz, _sz, _sz, C.c_int, C.c_double, _vp, _sz,
                                          C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_dev.argtypes = [_vp, _sz, C.c_int, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz),
                                            C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_box_dev.argtypes = [_vp, _sz, C.c_int, C.POINTER(_sz), C.POINTER(_sz), _vp, _sz, _vp]
    lib.sperrhip_multires_levels.argtypes = [_sz] * 6 + [C.POINTER(_sz), C.POINTER(_sz)]
    lib.sperrhip_decompress_multires_dev.argtypes = [_vp, _sz, C.c_int, _vp, _sz, _sz, _vp, _vp]
    return lib


def baseline_child(args):
    """child process: the other build, through its C ABI alone"""
    import torch
    lib = wire(C.CDLL(args.child))
    dev = torch.device("cuda", torch.cuda.current_device())
    S, ch = args.size, args.chunk
    vol = make_volume(torch, dev, S)
    mode, q = quality_of(torch, vol, args.case, args)
    st = _vp(torch.cuda.current_stream().cuda_stream)
    cap = lib.sperrhip_max_compressed_size(S, S, S, ch, ch, ch, mode, q)
    buf = torch.empty(cap, dtype=torch.uint8, device=dev)
    ln = _sz(0)
    assert lib.sperrhip_compress_dev(vol.data_ptr(), 1, S, S, S, ch, ch, ch, mode, q, buf.data_ptr(), cap, C.byref(ln),
                                     st) == 0
    torch.cuda.synchronize()
    del vol
    cont = buf[:ln.value].clone()
    del buf
    out = torch.empty(S * S * S, dtype=torch.float32, device=dev)
    d = [_sz(0) for _ in range(3)]

    def full():
        assert lib.sperrhip_decompress_dev(cont.data_ptr(), cont.numel(), 1, out.data_ptr(), out.numel() * 4,
                                           C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), st) == 0

    nlev, dims = _sz(0), (_sz * 48)()
    assert lib.sperrhip_multires_levels(S, S, S, ch, ch, ch, C.byref(nlev), dims) == 0
    lv = [torch.empty(dims[3 * k] * dims[3 * k + 1] * dims[3 * k + 2], dtype=torch.float64, device=dev)
          for k in range(nlev.value)]
    ptrs = (_vp * max(1, nlev.value))(*[t.data_ptr() for t in lv])

    def multires():
        assert lib.sperrhip_decompress_multires_dev(cont.data_ptr(), cont.numel(), 1, out.data_ptr(), out.numel() * 4,
                                                    nlev.value, ptrs, st) == 0

    lo, bd = (_sz * 3)(ch, ch, ch), (_sz * 3)(ch, ch, ch)

    def box():
        assert lib.sperrhip_decompress_box_dev(cont.data_ptr(), cont.numel(), 1, lo, bd, out.data_ptr(),
                                               ch * ch * ch * 4, st) == 0

    r = {"full": timed(torch, full, args.runs, args.warmup),
         "multires": timed(torch, multires, args.runs, args.warmup),
         "box_256_chunk": timed(torch, box, args.runs, args.warmup),
         "container_sha256": hashlib.sha256(cont.cpu().numpy().tobytes()).hexdigest()}
    print("BASELINE " + json.dumps(r), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--bpp", type=float, default=2.0)
    ap.add_argument("--pwe-rel", type=float, default=1e-3)
    ap.add_argument("--cases", default="fixed_rate,pwe")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_bench.json"))
    args = ap.parse_args()
    if args.child:
        return baseline_child(args)
    import torch

    from sperr_amd.api import SperrHip

    S, ch = args.size, args.chunk
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = SperrHip()
    results = []
    for case in args.cases.split(","):
        r = {"case": case}
        if args.baseline_lib:   # (first: the child has the device to itself, and this build's runs follow it)
            cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child",
                   os.path.abspath(args.baseline_lib), "--case", case, "--size", str(S), "--chunk", str(ch), "--bpp",
                   str(args.bpp), "--pwe-rel", str(args.pwe_rel), "--runs", str(args.runs), "--warmup",
                   str(args.warmup)]
            res = subprocess.run(cmd, capture_output=True, text=True)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("BASELINE ")]
            if res.returncode != 0 or not line:   # (nothing more is started on the device after a child that failed)
                sys.stderr.write(res.stdout + res.stderr)
                return 2
            r["baseline"] = json.loads(line[-1][len("BASELINE "):])
        vol = make_volume(torch, dev, S)
        mode, q = quality_of(torch, vol, case, args)
        r["mode"], r["quality"] = mode, q
        cont = eng.compress(vol, (ch, ch, ch), q, mode=mode).clone()
        del vol
        torch.cuda.empty_cache()
        r["bytes"] = cont.numel()
        if "baseline" in r:
            sha = hashlib.sha256(cont.cpu().numpy().tobytes()).hexdigest()
            r["baseline_container_equal"] = sha == r["baseline"].pop("container_sha256")
        levels = eng.multires_levels((S, S, S), (ch, ch, ch))
        grid = S // ch
        out = torch.empty(max(lz * ly * lx for lz, ly, lx in levels), dtype=torch.float32, device=dev)
        r["level_dims_zyx"] = [list(s) for s in levels]
        r["level"], r["level_box"] = [], []
        for h, (lz, ly, lx) in enumerate(levels):
            whole = out[:lz * ly * lx].view(lz, ly, lx)
            r["level"].append(timed(torch, lambda: eng.decompress_level(cont, h, output_float=True, out=whole),
                                    args.runs, args.warmup))
            c = (lx // grid, ly // grid, lz // grid)
            lo = tuple(min(1, grid - 1) * x for x in c)
            part = out[:c[0] * c[1] * c[2]].view(c[2], c[1], c[0])
            r["level_box"].append(timed(torch, lambda: eng.decompress_level(cont, h, lo, c, output_float=True, out=part),
                                        args.runs, args.warmup))
        one = out[:ch * ch * ch].view(ch, ch, ch) if out.numel() >= ch ** 3 else torch.empty((ch, ch, ch),
                                                                                           dtype=torch.float32, device=dev)
        lo = tuple(min(1, grid - 1) * ch for _ in range(3))
        r["box_256_chunk"] = timed(torch, lambda: eng.decompress_box(cont, lo, (ch, ch, ch), out=one), args.runs,
                                   args.warmup)
        if "baseline" in r:
            b = r["baseline"]
            r["levels_not_slower_than_baseline_full"] = [lv["max"] <= b["full"]["min"] for lv in r["level"]]
            r["level_boxes_not_slower_than_baseline_box"] = [lv["max"] <= b["box_256_chunk"]["min"]
                                                             for lv in r["level_box"]]
        print(json.dumps(r), flush=True)
        results.append(r)
        del cont, out
        torch.cuda.empty_cache()
    doc = {"metric": "level_decode_ms", "volume": [S, S, S], "chunks": [ch, ch, ch], "runs": args.runs,
           "warmup": args.warmup, "timing": "HIP events around the call: min / median / max of the runs",
           "device": torch.cuda.get_device_name(dev),
           "baseline_lib": os.path.basename(args.baseline_lib) if args.baseline_lib else None, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
