#!/usr/bin/env python3
"""series_bench.py -- what the time-series calls cost and what they buy, on one GPU.

  kernels   k_series_fwd and k_series_inv alone (the library's profiler brackets the launches with events) on 8 and 16
            steps of 256^3 and 512^3, fp32 and fp64, levels 3 and 4: time and share of the HBM peak with the steps once in
            and the bands once out (or back) as the bytes, beside the torch expressions they replace (the butterflies
            written with tensor slices, level by level)
  calls     compress_series / decompress_series against compress_batch / decompress_batch (mode 3, doubles of the same
            steps: what levels=0 is) on 16 steps of 256^3 in 64^3 chunks; one step of the 16-step series against one
            decompress; the staging memory (sperrhip_debug_counter(3) does not see it: the bands' bytes are stated)
  bytes     8 steps of 256^3 in 64^3 and in 256^3 chunks, the field drifting 0.05 / 0.25 / 1 samples a step (turbulence of
            period 64, and a Gaussian puff over weak turbulence, drifts 0 / 0.25 / 1): the series' bytes over the bytes
            of eight containers of the steps alone, at two tolerances and two PSNR targets.  Losses are reported as they
            come

Every time is the median (and min ... max) of --runs calls after --warmup, the sides of a comparison alternating run
by run, each timed with events on the current stream.

  python tools/series_bench.py [--runs 15] [--warmup 3] [--parts kernels,calls,bytes] [--out profiles/series_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8.0e12   # bytes per second
S = float.fromhex("0x1.6a09e667f3bcdp-1")


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def torch_forward(torch, steps, levels):
    """the forward butterflies of one group of 2^levels steps as tensor expressions: (g, ...) -> (g, ...) float64"""
    v = steps.to(torch.float64)
    length = v.shape[0]
    while length > 1:
        e, o = v[0:length:2], v[1:length:2]
        v = torch.cat([(e + o) * S, (e - o) * S, v[length:]])
        length //= 2
    return v


def torch_inverse(torch, bands, dtype):
    v = bands
    g = v.shape[0]
    length = 2
    while length <= g:
        a, d = v[:length // 2], v[length // 2:length]
        head = torch.stack([(a + d) * S, (a - d) * S], dim=1).reshape((length,) + tuple(v.shape[1:]))
        v = torch.cat([head, v[length:]])
        length *= 2
    return v.to(dtype)


def turbulence_at(torch, n, origin_xyz, period=64.0, seed=42, slab=32):
    """sperr_amd.synth.turbulence on the device with a real-valued origin"""
    from sperr_amd.synth import mode_table
    kv, ph, am = mode_table(seed)
    w = 2.0 * math.pi / period
    ax = torch.arange(n, dtype=torch.float64, device="cuda")
    x, y = (ax + origin_xyz[0]) * w, (ax + origin_xyz[1]) * w
    out = torch.empty((n, n, n), dtype=torch.float32, device="cuda")
    for z0 in range(0, n, slab):
        z = (ax[z0:z0 + slab] + origin_xyz[2]) * w
        acc = torch.zeros((z.numel(), n, n), dtype=torch.float64, device="cuda")
        for m in range(len(ph)):
            acc += am[m] * torch.sin((kv[m, 0] * x)[None, None, :] + (kv[m, 1] * y)[None, :, None] +
                                     (kv[m, 2] * z)[:, None, None] + ph[m])
        out[z0:z0 + slab] = acc.to(torch.float32)
    return out


def series_field(torch, name, n, nsteps, drift):
    if name == "turbulence":   # drifts along x; the origin also moves by 0.5 and 0.3 of that along y and z
        return [turbulence_at(torch, n, (drift * t, 0.5 * drift * t, 0.3 * drift * t)) for t in range(nsteps)]
    k = n / 32.0               # the puff of the 32^3 experiment, scaled with the volume
    ax = torch.arange(n, dtype=torch.float64, device="cuda")
    z, y, x = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    weak = 1e-3 * turbulence_at(torch, n, (0.0, 0.0, 0.0), seed=7).to(torch.float64)
    return [(torch.exp(-((x - 10 * k - drift * t) ** 2 + (y - 16 * k) ** 2 + (z - 16 * k) ** 2) / (30 * k * k)) + weak)
            .to(torch.float32) for t in range(nsteps)]


def part_kernels(torch, eng, args, rec):
    from size_bench import kernel_ms, timed
    out = rec.setdefault("kernels", {})
    for n in (256, 512):
        for nsteps in (8, 16):
            for dt in (torch.float32, torch.float64):
                levels = 3 if nsteps == 8 else 4
                g = torch.Generator(device="cuda").manual_seed(5)
                steps = torch.randn((nsteps, n, n, n), generator=g, device="cuda", dtype=dt)
                bands = torch.empty((nsteps, n, n, n), device="cuda", dtype=torch.float64)
                back = torch.empty_like(steps)
                nbytes = steps.numel() * (steps.element_size() + 8)
                fwd = kernel_ms(torch, eng, lambda: eng.series_forward(steps, levels, out=bands), "k_series_fwd",
                                args.runs, args.warmup)
                inv = kernel_ms(torch, eng, lambda: eng.series_inverse(bands, levels, output_float=dt == torch.float32,
                                                                       out=back), "k_series_inv", args.runs, args.warmup)
                r = {"bytes": nbytes, "levels": levels, "k_series_fwd": stats(fwd), "k_series_inv": stats(inv),
                     "k_series_fwd_fraction_of_hbm_peak": round(nbytes / (statistics.median(fwd) * 1e-3) / HBM_PEAK, 4),
                     "k_series_inv_fraction_of_hbm_peak": round(nbytes / (statistics.median(inv) * 1e-3) / HBM_PEAK, 4)}
                if n == 256:   # (the expressions hold several copies of the series)
                    ms = timed(torch, {"torch_forward": lambda: torch_forward(torch, steps, levels),
                                       "torch_inverse": lambda: torch_inverse(torch, bands, dt)}, args.runs, args.warmup)
                    r.update({k: stats(v) for k, v in ms.items()})
                    assert torch.equal(torch_forward(torch, steps, levels), bands)
                key = "%d steps of %d^3 %s" % (nsteps, n, str(dt).split(".")[-1])
                out[key] = r
                print(key, json.dumps(r), flush=True)
                del steps, bands, back
                torch.cuda.empty_cache()


def part_calls(torch, eng, args, rec):
    from size_bench import timed
    out = rec.setdefault("calls", {})
    n, nsteps, chunks, levels = 256, 16, (64, 64, 64), 4
    steps = series_field(torch, "turbulence", n, nsteps, 0.05)
    stacked = torch.stack(steps)
    doubles = stacked.to(torch.float64)
    tol = 1e-3 * float(stacked.max().double() - stacked.min().double())
    cap = eng.max_compressed_size_batch(nsteps, (n, n, n), chunks, tol, 3)
    buf_a = torch.empty(cap, dtype=torch.uint8, device="cuda")
    buf_b = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ms = timed(torch, {"compress_series": lambda: eng.compress_series(steps, chunks, tol=tol, levels=levels, out=buf_a),
                       "compress_batch_of_doubles": lambda: eng.compress_batch(doubles, chunks, tol, mode=3, out=buf_b),
                       "compress_batch_of_floats": lambda: eng.compress_batch(stacked, chunks, tol, mode=3, out=buf_b)},
               args.runs, args.warmup)
    r = {k: stats(v) for k, v in ms.items()}
    conts, info = eng.compress_series(steps, chunks, tol=tol, levels=levels, out=buf_a)
    plain = [c.clone() for c in eng.compress_batch(stacked, chunks, tol, mode=3, out=buf_b)]
    out_s = torch.empty((nsteps, n, n, n), dtype=torch.float32, device="cuda")
    out_b = torch.empty_like(out_s)
    one = torch.empty((1, n, n, n), dtype=torch.float32, device="cuda")
    ms = timed(torch, {"decompress_series": lambda: eng.decompress_series(conts, info, out=out_s),
                       "decompress_batch": lambda: eng.decompress_batch(plain, out=out_b),
                       "one_step_of_the_series": lambda: eng.decompress_series(conts, info, t0=5, nt=1, out=one),
                       "one_decompress": lambda: eng.decompress(plain[5], out=one[0])}, args.runs, args.warmup)
    r.update({k: stats(v) for k, v in ms.items()})
    worst = float((out_s.double() - stacked.double()).abs().max())
    r.update({"tol": tol, "worst_error_over_tol_fp32_output": round(worst / tol, 5),
              "series_bytes": sum(c.numel() for c in conts), "batch_bytes": sum(c.numel() for c in plain),
              "containers_one_step_needs": len(eng.series_needs(nsteps, levels, 5, 1)),
              "staging_bytes_compress": nsteps * n ** 3 * 8,
              "staging_bytes_one_step": len(eng.series_needs(nsteps, levels, 5, 1)) * n ** 3 * 8})
    out["16 steps of 256^3 in 64^3, turbulence drifting 0.05"] = r
    print(json.dumps(r), flush=True)


def part_bytes(torch, eng, args, rec):
    out = rec.setdefault("bytes", {})
    n, nsteps, levels = 256, 8, 3
    for name, drifts in (("turbulence", (0.05, 0.25, 1.0)), ("puff", (0.0, 0.25, 1.0))):
        for drift in drifts:
            steps = series_field(torch, name, n, nsteps, drift)
            stacked = torch.stack(steps)
            rng = float(stacked.max().double() - stacked.min().double())
            for ch in (64, 256):
                chunks = (ch, ch, ch)
                r = {}
                for rel in (1e-2, 1e-4):
                    s = sum(c.numel() for c in eng.compress_series(steps, chunks, tol=rel * rng, levels=levels)[0])
                    p = sum(eng.compress(v, chunks, rel * rng, mode=3).numel() for v in steps)
                    r["tol %g range" % rel] = {"series": s, "alone": p, "ratio": round(s / p, 3)}
                for psnr in (60.0, 100.0):
                    s = sum(c.numel() for c in eng.compress_series(steps, chunks, psnr=psnr, levels=levels)[0])
                    p = sum(eng.compress_to_psnr(v, chunks, psnr, range=rng).numel() for v in steps)
                    r["psnr %g dB" % psnr] = {"series": s, "alone": p, "ratio": round(s / p, 3)}
                key = "%s drifting %g, %d^3 chunks" % (name, drift, ch)
                out[key] = r
                print(key, json.dumps(r), flush=True)
            del steps, stacked
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="kernels,calls,bytes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_bench.json"))
    args = ap.parse_args()
    import torch
    from sperr_amd.api import SperrHip
    eng = SperrHip()
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rec.update({"runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)})
    for part in args.parts.split(","):
        {"kernels": part_kernels, "calls": part_calls, "bytes": part_bytes}[part](torch, eng, args, rec)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
