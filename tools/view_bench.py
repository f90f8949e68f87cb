#!/usr/bin/env python3
"""view_bench.py -- what a strided view saves: compress, whole decode and quality of the 1024^3 fp32 interior of a
padded device array (256^3 chunks, 2 bpp), by three routes each.

  view    the view call on the interior where it lies (sperrhip_compress_view_dev, _decompress_view_dev,
          _quality_view_dev)
  copy    what a caller did before there were views: .contiguous() copies, then the dense call (for the decode: the
          dense call, then a copy into the interior).  Timed in a child process on another build of the library
          (--parent-lib: the parent commit's), so that the figure is what that commit gave; without --parent-lib the
          child loads this build, and the JSON says so
  dense   the dense call on packed data, for reference (no copy; not what a halo array's owner can call)

Two parents: 1032 x 1030 x 1028 with the interior at (4, 3, 2) -- the row pitch and the first element are multiples of
16 bytes, so the conditioner streams rows (k_stride_sums_rows) -- and 1031 x 1030 x 1028 with the interior at (3, 3, 2):
an odd pitch, the conditioner's fallback (k_stride_sums).  Every route is timed with HIP events around it on the
current stream, median and min ... max of --runs runs after --warmup.  The gate earlier feature changes used: the
slowest view run is faster than the fastest run of the copy route.  view / dense is reported, not gated.

  python tools/view_bench.py [--runs 15] [--warmup 3] [--parent-lib PATH] [--out profiles/view_bench.json] [--small]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (as sperr_amd/api.py asks)
_sz, _vp = C.c_size_t, C.c_void_p
CHUNKS, BPP = (256, 256, 256), 2.0


class View(C.Structure):
    _fields_ = [("pitch_y", _sz), ("pitch_z", _sz)]


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


class Lib:
    """the C entry points of a build of the library, views where it has them"""

    def __init__(self, path):
        import torch   # (its HIP runtime first: sperr_amd/api.py, load_library)
        self.torch = torch
        lib = self.lib = C.CDLL(path)
        lib.sperrhip_max_compressed_size.restype = _sz
        lib.sperrhip_max_compressed_size.argtypes = [_sz] * 6 + [C.c_int, C.c_double]
        lib.sperrhip_compress_dev.argtypes = [_vp, C.c_int] + [_sz] * 6 + [C.c_int, C.c_double, _vp, _sz,
                                                                          C.POINTER(_sz), _vp]
        lib.sperrhip_decompress_dev.argtypes = [_vp, _sz, C.c_int, _vp, _sz] + [C.POINTER(_sz)] * 3 + [_vp]
        lib.sperrhip_quality_dev.argtypes = [_vp, _vp, C.c_int, _sz, C.POINTER(C.c_double), _vp]
        self.has_views = hasattr(lib, "sperrhip_compress_view_dev")
        if self.has_views:
            lib.sperrhip_compress_view_dev.argtypes = [_vp, C.POINTER(View), C.c_int] + [_sz] * 6 + \
                [C.c_int, C.c_double, _vp, _sz, C.POINTER(_sz), _vp]
            lib.sperrhip_decompress_view_dev.argtypes = [_vp, _sz, C.c_uint, C.c_int, C.POINTER(_sz), C.POINTER(_sz),
                                                         _vp, C.POINTER(View), _sz, _vp]
            lib.sperrhip_quality_view_dev.argtypes = [_vp, C.POINTER(View), _vp, C.POINTER(View), C.c_int, _sz, _sz,
                                                      _sz, C.POINTER(C.c_double), _vp]
        self.fig = (C.c_double * 8)()

    def stream(self):
        return _vp(self.torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def ok(rtn, what):
        if rtn != 0:
            raise RuntimeError(f"{what} returned {rtn}")

    def compress(self, vol, out, view=None):
        dz, dy, dx = vol.shape
        n = _sz(0)
        if view is None:
            self.ok(self.lib.sperrhip_compress_dev(vol.data_ptr(), 1, dx, dy, dz, *CHUNKS, 1, BPP, out.data_ptr(),
                                                   out.numel(), C.byref(n), self.stream()), "sperrhip_compress_dev")
        else:
            self.ok(self.lib.sperrhip_compress_view_dev(vol.data_ptr(), C.byref(view), 1, dx, dy, dz, *CHUNKS, 1, BPP,
                                                        out.data_ptr(), out.numel(), C.byref(n), self.stream()),
                    "sperrhip_compress_view_dev")
        return out[:n.value]

    def decompress(self, c, out, view=None):
        d = [_sz(0), _sz(0), _sz(0)]
        if view is None:
            self.ok(self.lib.sperrhip_decompress_dev(c.data_ptr(), c.numel(), 1, out.data_ptr(), out.numel() * 4,
                                                     C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), self.stream()),
                    "sperrhip_decompress_dev")
        else:
            room = out.untyped_storage().nbytes() - out.storage_offset() * 4
            self.ok(self.lib.sperrhip_decompress_view_dev(c.data_ptr(), c.numel(), 0, 1, None, None, out.data_ptr(),
                                                          C.byref(view), room, self.stream()),
                    "sperrhip_decompress_view_dev")

    def quality(self, a, b, va=None, vb=None):
        if va is None and vb is None:
            self.ok(self.lib.sperrhip_quality_dev(a.data_ptr(), b.data_ptr(), 1, a.numel(), self.fig, self.stream()),
                    "sperrhip_quality_dev")
        else:
            dz, dy, dx = a.shape
            self.ok(self.lib.sperrhip_quality_view_dev(a.data_ptr(), C.byref(va), b.data_ptr(), C.byref(vb), 1, dx, dy,
                                                       dz, self.fig, self.stream()), "sperrhip_quality_view_dev")
        return list(self.fig)


def layouts(n):
    """name -> (parent shape (z, y, x), interior origin (z, y, x))"""
    return {"pitch_16B": ((n + 4, n + 6, n + 8), (2, 3, 4)), "pitch_odd": ((n + 4, n + 6, n + 7), (2, 3, 3))}


def run(lib, n, runs, warmup, routes):
    """{layout: {op: {route: ms stats}}} of the routes asked for, with the checks that they computed the same"""
    import torch
    from sperr_amd.synth import turbulence_torch

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    packed = turbulence_torch((n, n, n), "cuda")
    cap = lib.lib.sperrhip_max_compressed_size(n, n, n, *CHUNKS, 1, BPP)
    cbuf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    container = lib.compress(packed, cbuf).clone()
    recon = torch.empty_like(packed)
    lib.decompress(container, recon)
    want_fig = lib.quality(packed, recon)
    scratch = torch.empty_like(packed)
    out = {}
    for name, (pshape, org) in layouts(n).items():
        sl = tuple(slice(o, o + n) for o in org)
        pa = torch.zeros(pshape, dtype=torch.float32, device="cuda")
        pb = torch.zeros(pshape, dtype=torch.float32, device="cuda")
        wa, wb = pa[sl], pb[sl]
        wa.copy_(packed)
        wb.copy_(recon)
        view = View(pshape[2], pshape[1] * pshape[2])
        fns = {}
        if "view" in routes:
            fns[("compress", "view")] = lambda: lib.compress(wa, cbuf, view)
            fns[("decode", "view")] = lambda: lib.decompress(container, wb, view)
            fns[("quality", "view")] = lambda: lib.quality(wa, wb, view, view)
        if "copy" in routes:
            fns[("compress", "copy")] = lambda: lib.compress(wa.contiguous(), cbuf)
            fns[("decode", "copy")] = lambda: (lib.decompress(container, scratch), wb.copy_(scratch))
            fns[("quality", "copy")] = lambda: lib.quality(wa.contiguous(), wb.contiguous())
        if "dense" in routes:
            fns[("compress", "dense")] = lambda: lib.compress(packed, cbuf)
            fns[("decode", "dense")] = lambda: lib.decompress(container, scratch)
            fns[("quality", "dense")] = lambda: lib.quality(packed, recon)
        ms = {k: [] for k in fns}
        for it in range(warmup + runs):
            for k, fn in fns.items():   # (the routes alternate, run by run)
                t = timed(fn)
                if it >= warmup:
                    ms[k].append(t)
        rec = {"parent_xyz": list(reversed(pshape)), "origin_xyz": list(reversed(org)),
               "first_element_16B_aligned": wa.data_ptr() % 16 == 0}
        for (op, route), v in ms.items():
            rec.setdefault(op, {})[route + "_ms"] = stats(v)
        # every route computed the same thing
        for route in routes:
            v = view if route == "view" else None
            src = wa if route in ("view",) else (wa.contiguous() if route == "copy" else packed)
            c = lib.compress(src, cbuf, v)
            assert torch.equal(c, container), (name, route, "container differs")
            if route == "view":
                wb.zero_()
                lib.decompress(container, wb, view)
                assert torch.equal(wb, recon), (name, "decode differs")
                assert lib.quality(wa, wb, view, view) == want_fig, (name, "figures differ")
        rec["checked"] = "containers, decoded interiors and figures equal the dense calls'"
        out[name] = rec
        del pa, pb, wa, wb
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libsperr_hip.so built from the parent commit")
    ap.add_argument("--small", action="store_true", help="a 128^3 interior: a rehearsal of the script")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)   # (the copy route on the library at this path)
    args = ap.parse_args()
    n = 128 if args.small else 1024
    here = os.path.join(ROOT, "sperr_amd", "libsperr_hip.so")

    if args.child:
        print(json.dumps(run(Lib(args.child), n, args.runs, args.warmup, ("copy",))))
        return

    import torch
    lib = Lib(here)
    res = run(lib, n, args.runs, args.warmup, ("view", "dense"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", args.parent_lib or here, "--runs", str(args.runs),
           "--warmup", str(args.warmup)] + (["--small"] if args.small else [])
    child = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if child.returncode != 0:
        raise RuntimeError("the copy route's process failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
    copy = json.loads(child.stdout.strip().splitlines()[-1])
    for name, rec in res.items():
        for op in ("compress", "decode", "quality"):
            rec[op].update(copy[name][op])
            v, c, d = rec[op]["view_ms"], rec[op]["copy_ms"], rec[op]["dense_ms"]
            rec[op]["view_max_below_copy_min"] = v["max"] < c["min"]
            rec[op]["copy_over_view"] = round(c["median"] / v["median"], 3)
            rec[op]["view_over_dense"] = round(v["median"] / d["median"], 3)
    # the conditioner's kernel per layout, and the kernels of the view calls, from the library's profiler
    from sperr_amd.api import SperrHip
    eng = SperrHip()
    for name, (pshape, org) in layouts(n).items():
        p = torch.zeros(pshape, dtype=torch.float32, device="cuda")
        w = p[tuple(slice(o, o + n) for o in org)]
        eng.compress(w, CHUNKS, BPP)
        eng.profile(True)
        eng.compress(w, CHUNKS, BPP)
        torch.cuda.synchronize()
        rep = eng.profile_report()
        eng.profile(False)
        res[name]["conditioner_ms"] = {k: round(v[0], 3) for k, v in rep.items() if k.startswith("k_stride_sums")}
        del p, w
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
           "interior": [n, n, n], "chunks": list(CHUNKS), "bpp": BPP, "dtype": "float32",
           "timing": "HIP events around the whole route, ms",
           "copy_route_build": "the parent commit's library, in a child process" if args.parent_lib
                               else "this build, in a child process",
           "layouts": res}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
