#!/usr/bin/env python3
"""fields_bench.py -- what the fields calls save: compress and decompress of four fp32 fields of 1024^3 kept
interleaved on the device, (z, y, x, 4), in 256^3 chunks at 2 bpp, by three routes each.

  fields   the new calls on the array where it lies (sperrhip_compress_fields_dev, sperrhip_decompress_fields_dev)
  torch    the only route before them: t.permute(3, 0, 1, 2).contiguous() then compress_batch; decompress_batch then
           out.permute(3, 0, 1, 2).copy_(stacked).  Timed in a child process on another build of the library
           (--parent-lib: the parent commit's), so that the figure is what that commit gave; without --parent-lib the
           child loads this build, and the JSON says so
  stacked  the batch call on data that already is stacked, for reference (no copy; not what an interleaved array's
           owner can call)

Every route is timed with HIP events around it on the current stream, the routes of a process alternating run by run;
median and min ... max of --runs runs after --warmup.  The gate earlier feature changes used, for compress and for
decompress: the slowest fields run is faster than the fastest torch run.

Reported, not gated (--extra-runs runs each, this build): three fields, eight fields, fields 1..2 of four, fp64 -- and
the two kernels alone, from the library's profiler, as bytes moved (the selected fields, read once and written once)
over kernel time, beside a device-to-device copy of as many bytes timed in the same run.

LDS bank conflicts come from a counters-only profiler run of its own:
  rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d DIR -o pmc -- \\
      python tools/fields_bench.py --pmc-workload
  python tools/fields_bench.py --merge-pmc DIR --out profiles/fields_bench.json
The workload launches, for stride_x 2, 3, 4 and 8 in that order, the 16-byte gather and scatter and then, one element
off alignment, the element forms; --merge-pmc matches the dispatches of every kernel to the strides by their order.

  python tools/fields_bench.py [--runs 15] [--warmup 3] [--parent-lib PATH] [--out profiles/fields_bench.json] [--small]
"""
import argparse
import csv
import ctypes as C
import glob
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
PMC_STRIDES = (2, 3, 4, 8)


class Fields(C.Structure):
    _fields_ = [("stride_x", _sz), ("pitch_y", _sz), ("pitch_z", _sz)]


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


class Lib:
    """the C entry points of a build of the library, the fields calls where it has them"""

    def __init__(self, path):
        import torch   # (its HIP runtime first: sperr_amd/api.py, load_library)
        self.torch = torch
        lib = self.lib = C.CDLL(path)
        lib.sperrhip_max_compressed_size_batch.restype = _sz
        lib.sperrhip_max_compressed_size_batch.argtypes = [_sz] * 7 + [C.c_int, C.c_double]
        lib.sperrhip_compress_batch_dev.argtypes = [_vp, C.c_int] + [_sz] * 7 + [C.c_int, C.c_double, _vp, _sz,
                                                                                C.POINTER(_sz), _vp]
        lib.sperrhip_decompress_batch_dev.argtypes = [_vp, C.POINTER(_sz), _sz, C.c_int, _vp, _sz] + \
            [C.POINTER(_sz)] * 3 + [_vp]
        self.has_fields = hasattr(lib, "sperrhip_compress_fields_dev")
        if self.has_fields:
            lib.sperrhip_compress_fields_dev.argtypes = [_vp, C.POINTER(Fields), _sz, C.c_int] + [_sz] * 6 + \
                [C.c_int, C.c_double, _vp, _sz, C.POINTER(_sz), _vp]
            lib.sperrhip_decompress_fields_dev.argtypes = [_vp, C.POINTER(_sz), _sz, C.c_int, _sz, _sz, _sz, _vp,
                                                           C.POINTER(Fields), _sz, _vp]

    def stream(self):
        return _vp(self.torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def ok(rtn, what):
        if rtn != 0:
            raise RuntimeError(f"{what} returned {rtn}")

    def cap(self, nf, n):
        return self.lib.sperrhip_max_compressed_size_batch(nf, n, n, n, *CHUNKS, 1, BPP)

    def compress_batch(self, stacked, out):
        """stacked (nf, z, y, x) -> (the containers' bytes, their offsets)"""
        nf, dz, dy, dx = stacked.shape
        offs = (_sz * (nf + 1))()
        self.ok(self.lib.sperrhip_compress_batch_dev(stacked.data_ptr(), int(stacked.element_size() == 4), nf, dx, dy,
                                                     dz, *CHUNKS, 1, BPP, out.data_ptr(), out.numel(), offs,
                                                     self.stream()), "sperrhip_compress_batch_dev")
        return out[:offs[nf]], offs

    def decompress_batch(self, c, offs, stacked):
        d = [_sz(0), _sz(0), _sz(0)]
        self.ok(self.lib.sperrhip_decompress_batch_dev(c.data_ptr(), offs, stacked.shape[0],
                                                       int(stacked.element_size() == 4), stacked.data_ptr(),
                                                       stacked.numel() * stacked.element_size(), C.byref(d[0]),
                                                       C.byref(d[1]), C.byref(d[2]), self.stream()),
                "sperrhip_decompress_batch_dev")

    @staticmethod
    def layout(t):
        """the layout of a (z, y, x, f) tensor with unit field stride"""
        return Fields(t.stride(2), t.stride(1), t.stride(0))

    def compress_fields(self, t, out):
        dz, dy, dx, nf = t.shape
        offs = (_sz * (nf + 1))()
        self.ok(self.lib.sperrhip_compress_fields_dev(t.data_ptr(), C.byref(self.layout(t)), nf,
                                                      int(t.element_size() == 4), dx, dy, dz, *CHUNKS, 1, BPP,
                                                      out.data_ptr(), out.numel(), offs, self.stream()),
                "sperrhip_compress_fields_dev")
        return out[:offs[nf]], offs

    def decompress_fields(self, c, offs, t):
        dz, dy, dx, nf = t.shape
        room = t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()
        self.ok(self.lib.sperrhip_decompress_fields_dev(c.data_ptr(), offs, nf, int(t.element_size() == 4), dx, dy, dz,
                                                        t.data_ptr(), C.byref(self.layout(t)), room, self.stream()),
                "sperrhip_decompress_fields_dev")


def make_fields(n, nrec, dtype):
    """(z, y, x, nrec) interleaved on the device: one turbulence volume, scaled, shifted and rolled per field"""
    import torch
    from sperr_amd.synth import turbulence_torch
    base = turbulence_torch((n, n, n), "cuda", dtype=dtype)
    t = torch.empty((n, n, n, nrec), dtype=dtype, device="cuda")
    for f in range(nrec):
        t[..., f] = torch.roll(base, shifts=17 * f, dims=f % 3) * float(10 ** (f % 4)) + float(f)
    del base
    return t


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, runs, warmup):
    ms = {k: [] for k in fns}
    for it in range(warmup + runs):
        for k, fn in fns.items():   # (the routes alternate, run by run)
            t = timed(fn)
            if it >= warmup:
                ms[k].append(t)
    return {k: stats(v) for k, v in ms.items()}


def run_case(lib, n, nrec, first, nf, dtype, runs, warmup, routes):
    """{op: {route_ms: stats}} for fields [first, first + nf) of an nrec-wide record, and a check that the routes
    computed the same"""
    import torch
    whole = make_fields(n, nrec, dtype)
    t = whole[..., first:first + nf]
    stacked = t.permute(3, 0, 1, 2).contiguous()
    cbuf = torch.empty(lib.cap(nf, n), dtype=torch.uint8, device="cuda")
    back = torch.empty_like(stacked)
    target = torch.zeros_like(whole)
    tv = target[..., first:first + nf]
    # The engine sizes its workspace against the memory that is free at its first call: every tensor of the case
    # exists by then, the torch route's packed copy is a block torch's allocator already holds, and the fields call
    # goes first, so that its staging buffer is there before the workspace is
    if "torch" in routes:
        warm = torch.empty_like(stacked)
        del warm
    c, offs = lib.compress_fields(t, cbuf) if "fields" in routes else lib.compress_batch(stacked, cbuf)
    container = c.clone()
    fns = {}
    if "fields" in routes:
        fns[("compress", "fields")] = lambda: lib.compress_fields(t, cbuf)
        fns[("decompress", "fields")] = lambda: lib.decompress_fields(container, offs, tv)
    if "torch" in routes:
        fns[("compress", "torch")] = lambda: lib.compress_batch(t.permute(3, 0, 1, 2).contiguous(), cbuf)
        fns[("decompress", "torch")] = lambda: (lib.decompress_batch(container, offs, back),
                                                tv.permute(3, 0, 1, 2).copy_(back))
    if "stacked" in routes:
        fns[("compress", "stacked")] = lambda: lib.compress_batch(stacked, cbuf)
        fns[("decompress", "stacked")] = lambda: lib.decompress_batch(container, offs, back)
    rec = {"record": nrec, "first": first, "nfields": nf, "dtype": str(dtype).split(".")[-1],
           "first_element_16B_aligned": t.data_ptr() % 16 == 0}
    for (op, route), v in alternate(fns, runs, warmup).items():
        rec.setdefault(op, {})[route + "_ms"] = v
    # every route computed the same thing
    c2, offs2 = lib.compress_batch(stacked, cbuf)
    assert list(offs2) == list(offs) and torch.equal(c2, container), "containers differ"
    lib.decompress_batch(container, offs, back)
    if "fields" in routes:
        c2, offs2 = lib.compress_fields(t, cbuf)
        assert list(offs2) == list(offs) and torch.equal(c2, container), "containers differ"
        target.zero_()
        lib.decompress_fields(container, offs, tv)
        assert torch.equal(tv.permute(3, 0, 1, 2), back), "decodes differ"
        tv.zero_()
        assert not bool(target.any()), "a field that was not selected was written"
    if "torch" in routes:
        c2, offs2 = lib.compress_batch(t.permute(3, 0, 1, 2).contiguous(), cbuf)
        assert list(offs2) == list(offs) and torch.equal(c2, container), "containers differ"
    rec["checked"] = "containers and decoded fields equal the batch calls' on stacked copies"
    del whole, t, stacked, cbuf, container, back, target, tv, c, c2, fns
    torch.cuda.empty_cache()
    lib.lib.sperrhip_release()   # (the next case sizes the engine's workspace against what is free then)
    print(f"[fields_bench] {routes}: {json.dumps(rec)}", file=sys.stderr, flush=True)
    return rec


def kernels_alone(n, nrec, first, nf, dtype, reps=7):
    """the two kernels from the library's profiler, and a device-to-device copy of the same bytes"""
    import torch
    from sperr_amd.api import SperrHip
    eng = SperrHip()
    whole = make_fields(n, nrec, dtype)
    t = whole[..., first:first + nf]
    stacked = torch.empty((nf,) + tuple(t.shape[:3]), dtype=dtype, device="cuda")
    nbytes = 2 * stacked.numel() * stacked.element_size()
    out = {"bytes_moved": nbytes}
    for name, fn in (("k_fields_gather", lambda: eng.fields_gather(t, out=stacked)),
                     ("k_fields_scatter", lambda: eng.fields_scatter(stacked, t))):
        fn()
        ms, form = [], None
        for _ in range(reps):
            eng.profile(True)
            fn()
            torch.cuda.synchronize()
            for k, (busy, launches) in eng.profile_report().items():
                if name in k and launches:
                    ms.append(busy / launches)
                    form = k
            eng.profile(False)
        med = statistics.median(ms)
        out[name] = {"form": form, "ms": stats(ms), "GB_per_s": round(nbytes / med / 1e6, 1)}
    other = torch.empty_like(stacked)
    copy = [timed(lambda: other.copy_(stacked)) for _ in range(reps + 2)][2:]
    out["device_copy_same_bytes"] = {"ms": stats(copy), "GB_per_s": round(nbytes / statistics.median(copy) / 1e6, 1)}
    del whole, t, stacked, other
    torch.cuda.empty_cache()
    eng.release()
    return out


def pmc_workload(n):
    import torch
    from sperr_amd.api import SperrHip
    eng = SperrHip()
    for stride in PMC_STRIDES:
        parent = torch.randn(n * n * n * stride + 4, dtype=torch.float32, device="cuda")
        stacked = torch.empty((stride, n, n, n), dtype=torch.float32, device="cuda")
        for lead in (0, 1):   # the 16-byte forms, then the element forms
            t = parent[lead:lead + n * n * n * stride].view(n, n, n, stride)
            eng.fields_gather(t, out=stacked)
            eng.fields_scatter(stacked, t)
        torch.cuda.synchronize()


def merge_pmc(d, out_path):
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    per = {}   # kernel -> dispatch id -> {counter: value}
    for r in rows:
        k = r["Kernel_Name"]
        if "k_fields_" not in k:
            continue
        per.setdefault(k, {}).setdefault(int(r["Dispatch_Id"]), {})
        c = per[k][int(r["Dispatch_Id"])]
        c[r["Counter_Name"]] = c.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    res = {}
    for k, disp in per.items():
        ids = sorted(disp)
        if len(ids) != len(PMC_STRIDES):
            raise RuntimeError(f"{k}: {len(ids)} dispatches, {len(PMC_STRIDES)} strides")
        short = ("k_fields_gather" if "gather" in k else "k_fields_scatter") + \
                ("<float, kVec>" if "Lb1" in k or "true" in k else "<float, element>")
        for stride, i in zip(PMC_STRIDES, ids):
            conf, act = disp[i].get("SQ_LDS_BANK_CONFLICT", 0.0), disp[i].get("SQ_LDS_IDX_ACTIVE", 0.0)
            res.setdefault(short, {})[f"stride_{stride}"] = {
                "SQ_LDS_BANK_CONFLICT": conf, "SQ_LDS_IDX_ACTIVE": act,
                "conflict_over_active": round(conf / act, 4) if act else None}
    with open(out_path) as f:
        doc = json.load(f)
    doc["lds_bank_conflicts"] = {"how": "rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE, a run of its own; "
                                        "fp32, nfields = stride_x, one launch per stride and form", "kernels": res}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["lds_bank_conflicts"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--extra-runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libsperr_hip.so built from the parent commit")
    ap.add_argument("--small", action="store_true", help="128^3 fields: a rehearsal of the script")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)   # (the torch route on the library at this path)
    ap.add_argument("--pmc-workload", action="store_true", help="only launch the kernels, for a counters run")
    ap.add_argument("--merge-pmc", default=None, help="directory of a rocprofv3 --pmc run to merge into --out")
    args = ap.parse_args()
    n = 128 if args.small else 1024
    here = os.path.join(ROOT, "sperr_amd", "libsperr_hip.so")
    if args.merge_pmc:
        merge_pmc(args.merge_pmc, args.out)
        return
    if args.pmc_workload:
        pmc_workload(128 if args.small else 256)
        return

    import torch
    if args.child:
        print(json.dumps(run_case(Lib(args.child), n, 4, 0, 4, torch.float32, args.runs, args.warmup, ("torch",))))
        return

    lib = Lib(here)
    gate = run_case(lib, n, 4, 0, 4, torch.float32, args.runs, args.warmup, ("fields", "stacked"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", args.parent_lib or here, "--runs", str(args.runs),
           "--warmup", str(args.warmup)] + (["--small"] if args.small else [])
    child = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if child.returncode != 0:
        raise RuntimeError("the torch route's process failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
    other = json.loads(child.stdout.strip().splitlines()[-1])
    verdict = True
    for op in ("compress", "decompress"):
        gate[op].update(other[op])
        f, t, s = gate[op]["fields_ms"], gate[op]["torch_ms"], gate[op]["stacked_ms"]
        gate[op]["fields_max_below_torch_min"] = f["max"] < t["min"]
        gate[op]["torch_over_fields"] = round(t["median"] / f["median"], 3)
        gate[op]["fields_over_stacked"] = round(f["median"] / s["median"], 3)
        verdict = verdict and gate[op]["fields_max_below_torch_min"]
    gate["kernels_alone"] = kernels_alone(n, 4, 0, 4, torch.float32)

    extras = {}
    for name, (nrec, first, nf, dt) in {"three_fields": (3, 0, 3, torch.float32), "eight_fields": (8, 0, 8, torch.float32),
                                        "fields_1_2_of_four": (4, 1, 2, torch.float32),
                                        "four_fields_fp64": (4, 0, 4, torch.float64)}.items():
        rec = run_case(lib, n, nrec, first, nf, dt, args.extra_runs, 1, ("fields", "torch", "stacked"))
        for op in ("compress", "decompress"):
            rec[op]["torch_over_fields"] = round(rec[op]["torch_ms"]["median"] / rec[op]["fields_ms"]["median"], 3)
        rec["kernels_alone"] = kernels_alone(n, nrec, first, nf, dt)
        rec["torch_route_build"] = "this build, same process"
        extras[name] = rec
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
           "extra_runs": args.extra_runs, "volume": [n, n, n], "chunks": list(CHUNKS), "bpp": BPP,
           "timing": "HIP events around the whole route, ms",
           "torch_route_build": "the parent commit's library, in a child process" if args.parent_lib
                                else "this build, in a child process",
           "gate": "four fp32 fields, aligned: the slowest fields run is faster than the fastest torch run, for "
                   "compress and for decompress",
           "gate_passed": verdict, "four_fields_fp32": gate, "reported_not_gated": extras}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
