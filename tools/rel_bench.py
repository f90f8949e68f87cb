#!/usr/bin/env python3
"""rel_bench.py -- what point-wise relative error costs, on one GPU.

  kernels     n^3 (512) fp32 and fp64: rel_forward and rel_inverse as calls, and k_rel_forward / k_rel_inverse alone (the
              library's profiler brackets each launch with events), against the torch passes they replace -- frexp,
              signbit, == 0 and back; and the same for the LOG map kind (map="log": k_rel_log_forward /
              k_rel_log_inverse, which add some forty fp64 operations a sample to the same traffic), each with its ratio
              to the linear kind's kernel of the same run.  The kernels move 12 (fp32) or 16 (fp64) bytes a sample forward and 12 or 16 back
              (8 of y', 4 or 8 of x'; the bit streams are a sixty-fourth of that); reported as a fraction of the HBM peak.
              The forward CALL also surveys y for its zeros, packs two streams and copies y to the caller.
  composites  m^3 (256): compress_rel / decompress_rel against compress in mode 3 at t / decompress of the same y
              volume, in-filled, already resident as doubles: the difference is the feature's cost
  kinks       on the same synthetic field (six decades, both signs) at eps 1e-2 and 1e-4, three containers: compress_rel
              of the linear kind, compress_rel of the log kind, and mode 3 on log2|x| computed by torch at the
              tolerance log2(1 + eps) -- what the piecewise linear logarithm costs against the true one, and that the
              library's own log kind collects it.  A record, no pass criterion.

Every time is the median (and min ... max) of --runs calls after --warmup, each timed with events on the current stream
around the call alone; the sides of a comparison alternate run by run.

  python tools/rel_bench.py [--runs 15] [--warmup 3] [--n 512] [--m 256] [--out profiles/rel_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # bytes per second


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


def kernel_ms(torch, eng, fn, kernel, runs, warmup):
    """[ms] of the launches of `kernel` inside fn, one per run"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        eng.profile(True)
        fn()
        torch.cuda.synchronize()
        rep = eng.profile_report(with_sum=True)
        eng.profile(False)
        hits = [v for k, v in rep.items() if kernel in k and v[1] > 0]   # (a template's name carries its arguments)
        assert hits and sum(h[1] for h in hits) == 1, rep
        out.append(sum(h[2] for h in hits))
    return out


def synthetic(torch, n, dtype):
    """six decades, both signs, smooth in the exponent, with a ball of zeros: a field like a mixing ratio's"""
    ax = torch.arange(n, device="cuda", dtype=torch.float64) * (2.0 * math.pi / n)
    z, y, x = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    expo = 3.0 * (torch.sin(1.3 * x + 0.2) * torch.cos(0.9 * y) + 0.6 * torch.sin(0.7 * z + 1.0) * torch.cos(2.1 * x + y))
    expo = expo.clamp(-3.0, 3.0)
    wave = torch.sin(3.1 * x + 2.3 * y + 1.7 * z) + 0.05 * torch.sin(17.0 * x) * torch.sin(13.0 * y + z)
    v = torch.pow(10.0, expo) * (1.0 + 0.3 * wave)
    v = torch.where(torch.cos(1.1 * x + 0.4 * z) * torch.sin(0.8 * y + 0.3) > -0.2, v, -v)
    c = torch.arange(n, device="cuda", dtype=torch.float64) - n / 2
    v[(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= (n / 8) ** 2] = 0.0
    return v.to(dtype).contiguous()


def torch_forward(torch, v):
    """what the forward kernel replaces: the exponent and mantissa, the sign bits, the zeros"""
    m, e = torch.frexp(v.to(torch.float64))
    y = (e - 1).to(torch.float64) + (2.0 * m.abs() - 1.0)
    return y, torch.signbit(v), v == 0


def torch_inverse(torch, y, neg, zero, dtype):
    e = torch.floor(y)
    a = torch.ldexp(1.0 + (y - e), e.to(torch.int32)).to(dtype)
    a = torch.where(zero, torch.zeros_like(a), a)
    return torch.where(neg, -a, a)


def bench_kernels(torch, eng, n, runs, warmup):
    out = {}
    for name, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
        v = synthetic(torch, n, dtype)
        nsamp, esz = v.numel(), v.element_size()
        y, side, nzero, nneg = eng.rel_forward(v)
        ylog, slog, _, _ = eng.rel_forward(v, map="log")
        ty, tneg, tzero = torch_forward(torch, v)
        back = torch.empty_like(v)
        isf = dtype == torch.float32
        calls = {"rel_forward": lambda: eng.rel_forward(v), "rel_forward_log": lambda: eng.rel_forward(v, map="log"),
                 "torch_forward": lambda: torch_forward(torch, v),
                 "rel_inverse": lambda: eng.rel_inverse(y, side, output_float=isf, out=back),
                 "rel_inverse_log": lambda: eng.rel_inverse(ylog, slog, output_float=isf, out=back),
                 "torch_inverse": lambda: torch_inverse(torch, ty, tneg, tzero, dtype)}
        ms = timed(torch, calls, runs, warmup)
        rec = {k: stats(vv) for k, vv in ms.items()}
        fwd_bytes, inv_bytes = nsamp * (esz + 8) + nsamp // 8, nsamp * (8 + esz) + nsamp // 4
        for kernel, fn, nbytes in (("k_rel_forward", calls["rel_forward"], fwd_bytes),
                                   ("k_rel_log_forward", calls["rel_forward_log"], fwd_bytes),
                                   ("k_rel_inverse", calls["rel_inverse"], inv_bytes),
                                   ("k_rel_log_inverse", calls["rel_inverse_log"], inv_bytes)):
            k = stats(kernel_ms(torch, eng, fn, kernel, runs, warmup))
            k["bytes"] = nbytes
            k["TB_per_s"] = round(nbytes / (k["median"] * 1e-3) / 1e12, 3)
            k["fraction_of_hbm_peak"] = round(nbytes / (k["median"] * 1e-3) / HBM_PEAK, 3)
            rec[kernel] = k
        for way in ("forward", "inverse"):
            rec["log_over_linear_" + way] = round(rec["k_rel_log_" + way]["median"] / rec["k_rel_" + way]["median"], 3)
        rec["samples"], rec["zeros"], rec["negative"], rec["side_bytes"] = nsamp, nzero, nneg, side.numel()
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
        del v, y, side, ylog, slog, ty, tneg, tzero, back
        eng.release()
        torch.cuda.empty_cache()
    return out


def bench_composites(torch, eng, m, runs, warmup):
    out = {}
    chunks = (min(m, 256),) * 3
    v = synthetic(torch, m, torch.float32)
    for eps in (1e-2, 1e-4):
        t = eng.rel_tolerance(eps, True)
        container, side = eng.compress_rel(v, chunks, eps)
        # the same y volume, in-filled as the call in-fills it, resident as doubles
        y, _, _, _ = eng.rel_forward(v)
        filled = torch.empty_like(y)
        eng.mask_make(y, "nan", filled_out=filled, fill="smooth")
        dense = eng.compress(filled, chunks, t, mode=3)
        assert bytes(dense.cpu().numpy()) == bytes(container.cpu().numpy())
        lcont, lside = eng.compress_rel(v, chunks, eps, map="log")
        calls = {"compress_rel": lambda: eng.compress_rel(v, chunks, eps),
                 "compress_rel_log": lambda: eng.compress_rel(v, chunks, eps, map="log"),
                 "compress_mode3_of_y": lambda: eng.compress(filled, chunks, t, mode=3),
                 "decompress_rel": lambda: eng.decompress_rel(container, side),
                 "decompress_rel_log": lambda: eng.decompress_rel(lcont, lside),
                 "decompress_of_y": lambda: eng.decompress(dense, output_float=False)}
        ms = timed(torch, calls, runs, warmup)
        rec = {k: stats(vv) for k, vv in ms.items()}
        rec["compress_cost_ms"] = round(rec["compress_rel"]["median"] - rec["compress_mode3_of_y"]["median"], 3)
        rec["decompress_cost_ms"] = round(rec["decompress_rel"]["median"] - rec["decompress_of_y"]["median"], 3)
        recon = eng.decompress_rel(container, side)
        worst, viol, mis, cnt = eng.rel_check(v, recon, eps)
        rec.update(t=t, container_bytes=container.numel(), side_bytes=side.numel(), input_bytes=v.numel() * 4,
                   worst_relative_error=worst, violations=viol, class_mismatches=mis)
        # the kinks: mode 3 on the true logarithm of the same samples, the zeros in-filled the same way
        tl = math.log2(1.0 + eps)
        ylog = torch.log2(v.to(torch.float64).abs())
        ylog[v == 0] = float("nan")
        flog = torch.empty_like(ylog)
        eng.mask_make(ylog, "nan", filled_out=flog, fill="smooth")
        clog = eng.compress(flog, chunks, tl, mode=3)
        rec.update(true_log_tolerance=tl, true_log_container_bytes=clog.numel(),
                   kink_ratio=round(container.numel() / clog.numel(), 4))
        # the library's own log kind: its container, its guarantee
        lworst, lviol, lmis, _ = eng.rel_check(v, eng.decompress_rel(lcont, lside), eps)
        rec.update(log_kind_t=eng.rel_tolerance(eps, True, map="log"), log_kind_container_bytes=lcont.numel(),
                   log_kind_side_bytes=lside.numel(), linear_over_log_kind=round(container.numel() / lcont.numel(), 4),
                   log_kind_worst_relative_error=lworst, log_kind_violations=lviol, log_kind_class_mismatches=lmis)
        out["eps_%g" % eps] = rec
        print("eps", eps, json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rel_bench.json"))
    args = ap.parse_args()
    import torch
    from sperr_amd.api import SperrHip
    eng = SperrHip()
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK,
           "kernels_%d_cubed" % args.n: bench_kernels(torch, eng, args.n, args.runs, args.warmup),
           "composites_%d_cubed_fp32" % args.m: bench_composites(torch, eng, args.m, args.runs, args.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
