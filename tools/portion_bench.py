#!/usr/bin/env python3
"""portion_bench.py -- what decoding a portion costs, and what truncating on the device costs.

The bench volume (1024^3 fp32 from sperr_amd/synth.py, 256^3 chunks, 2 bits per sample).  Device calls are timed with
HIP events around the call on the current stream, host entry points (they return host memory) with the wall clock;
every figure is the median and the min ... max of --runs runs after --warmup.  Two calls that are compared are timed
alternately, run by run, in this one process.  One JSON line on stdout (and in --out when given); per pct:

  device.portion      sperrhip_decompress_portion_dev on the whole container
  device.truncated    sperrhip_decompress_dev on what sperrhip_trunc_dev made of it (the same kernels, the same lengths)
  host.portion        sperrhip_decomp_3d_portion on the host container (uploads the kept prefixes only)
  host.farm           sperrhip_decomp_3d_farm on the host-truncated container (sperr_trunc_3d)
  trunc.call          sperrhip_trunc_dev, the whole call (two header read-backs, one upload, one kernel)
  trunc.kernel_ms     k_trunc_container alone (the library's profiler, runs of their own)
  trunc.copy          torch's device-to-device copy of as many bytes as the truncation writes
  GB/s                (bytes read + bytes written) / time = 2 x the output's length / time, for all three

  python tools/portion_bench.py [--size 1024] [--runs 15] [--warmup 3] [--host-runs N] [--out profiles/portion_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_sz, _vp = C.c_size_t, C.c_void_p


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--bpp", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=None, help="runs of the host entry points (default: --runs)")
    ap.add_argument("--host-warmup", type=int, default=None)
    ap.add_argument("--pcts", type=int, nargs="+", default=[100, 50, 25, 10])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from sperr_amd.api import SperrHip
    from sperr_amd.synth import turbulence_torch

    S, CH = args.size, args.chunk
    hruns = args.runs if args.host_runs is None else args.host_runs
    hwarm = args.warmup if args.host_warmup is None else args.host_warmup
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = SperrHip()
    vol = turbulence_torch((S, S, S), dev, seed=42)
    container = eng.compress(vol, (CH, CH, CH), args.bpp).clone()
    del vol
    host = container.cpu().numpy()
    out = torch.empty((S, S, S), dtype=torch.float32, device=dev)
    cut_buf = torch.empty(container.numel(), dtype=torch.uint8, device=dev)
    copy_src = torch.empty(container.numel(), dtype=torch.uint8, device=dev)
    copy_dst = torch.empty(container.numel(), dtype=torch.uint8, device=dev)
    libc = C.CDLL(None)
    libc.free.argtypes = [_vp]

    def ev_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall_ms(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def alternately(fns, clock, runs, warmup):
        """{name: [ms per run]}: every run times each of `fns` once, in order"""
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        ms = {k: [] for k in fns}
        for _ in range(runs):
            for k, fn in fns.items():
                ms[k].append(clock(fn))
        return ms

    def host_portion(pct):
        dst, od = _vp(None), (_sz * 3)()
        rc = eng.lib.sperrhip_decomp_3d_portion(host.ctypes.data, host.size, pct, 1, None, None, None, od, C.byref(dst))
        assert rc == 0, rc
        libc.free(dst)

    def host_farm(cut):
        dst, d = _vp(None), [_sz(0) for _ in range(3)]
        rc = eng.lib.sperrhip_decomp_3d_farm(cut.ctypes.data, cut.size, 1, 0, None, 0, C.byref(d[0]), C.byref(d[1]),
                                             C.byref(d[2]), C.byref(dst))
        assert rc == 0, rc
        libc.free(dst)

    res = {}
    for pct in args.pcts:
        cut = eng.truncate(container, pct, out=cut_buf)
        n = cut.numel()
        r = {"kept_bytes": n}
        ms = alternately({"portion": lambda: eng.decompress(container, True, out=out, pct=pct),
                          "truncated": lambda: eng.decompress(cut, True, out=out)}, ev_ms, args.runs, args.warmup)
        r["device"] = {k: stats(v) for k, v in ms.items()}
        a, b = r["device"]["portion"], r["device"]["truncated"]
        r["device"]["medians_inside_each_others_range"] = bool(b["min"] <= a["median"] <= b["max"] and
                                                               a["min"] <= b["median"] <= a["max"])
        if hruns > 0:
            hcut = np.frombuffer(eng.trunc_3d(host.tobytes(), pct), dtype=np.uint8)
            assert hcut.size == n
            ms = alternately({"portion": lambda: host_portion(pct), "farm": lambda: host_farm(hcut)}, wall_ms, hruns, hwarm)
            r["host"] = {k: stats(v) for k, v in ms.items()}
            r["host"]["runs"] = hruns
        # the truncation itself beside a copy of as many bytes
        ms = alternately({"call": lambda: eng.truncate(container, pct, out=cut_buf),
                          "copy": lambda: copy_dst[:n].copy_(copy_src[:n])}, ev_ms, args.runs, args.warmup)
        kern = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            eng.profile(True, only="k_trunc_container")
            eng.truncate(container, pct, out=cut_buf)
            kern.append(eng.profile_report().get("k_trunc_container", (0.0, 0))[0])
            eng.profile(False)
        ms["kernel"] = kern
        r["trunc"] = {k: dict(stats(v), **{"GB/s": round(2 * n / (statistics.median(v) * 1e-3) / 1e9, 1)})
                      for k, v in ms.items()}
        res[str(pct)] = r
    line = {"metric": "portion_ms", "volume": [S, S, S], "chunks": [CH, CH, CH], "bpp": args.bpp,
            "container_bytes": container.numel(), "runs": args.runs, "warmup": args.warmup, "pct": res,
            "device": torch.cuda.get_device_name(dev)}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
