#!/usr/bin/env python3
"""size_bench.py -- what compression to a byte target costs and what it buys, on one GPU.

  calls     n^3 fp32 (256 and 512) in 256^3 / 128^3 chunks: compress_to_size at a target of `--bpp` bits per sample
            against compress(mode=1) at that rate, and size_survey alone.  compress_to_size runs the float stages and
            the coder's head twice (the survey, then the encode) and reads the table back in between.
  kernel    k_lis_bits alone (the library's profiler brackets each launch with events), summed over the depths of
            one call, against the bytes it reads: a byte of M per node and one of its parent's, four of E per chain head
            -- counted here as 2 bytes a node, 1 / 8 node a sample: a lower bound on the traffic, so the fraction of the
            HBM peak is one too
  gain      PSNR of the dealt container against the fixed-rate container at the smallest rate that is at least as
            long: a turbulence-like field (sperr_amd.synth.turbulence_torch: homogeneous, like tests/golden/vort_crop.f32),
            and a plume (a Gaussian puff in a background a thousand times weaker) -- at 0.5, 1 and 2 bits per sample

Every time is the median (and min ... max) of --runs calls after --warmup, each timed with events on the current stream
around the call alone; the sides of a comparison alternate run by run.

  python tools/size_bench.py [--runs 15] [--warmup 3] [--bpp 2.0] [--sizes 256,512] [--out profiles/size_bench.json]
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
    """[ms] of all launches of `kernel` inside fn, summed, one figure per run"""
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
        hits = [v for k, v in rep.items() if kernel in k and v[1] > 0]
        assert hits, rep
        out.append(sum(h[2] for h in hits))
    return out


def plume_field(torch, n):
    """a Gaussian puff with fine structure in a background a thousand times weaker"""
    ax = torch.arange(n, device="cuda", dtype=torch.float64) / n
    z, y, x = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    r2 = (x - 0.3) ** 2 + (y - 0.35) ** 2 + (z - 0.25) ** 2
    puff = torch.exp(-r2 / (2 * 0.08 ** 2)) * (1.0 + 0.3 * torch.sin(40.0 * x + 31.0 * y) * torch.cos(27.0 * z))
    g = torch.Generator(device="cuda").manual_seed(11)
    back = 1e-3 * (torch.sin(9.0 * x + 4.0 * z) * torch.cos(7.0 * y) + 0.3 * torch.randn((n, n, n), generator=g, device="cuda", dtype=torch.float64))
    return (puff + back).to(torch.float32).contiguous()


def psnr(torch, eng, vol, container):
    back = eng.decompress(container, output_float=True)
    d = back.to(torch.float64) - vol.to(torch.float64)
    rng = float(vol.max() - vol.min())
    return 10.0 * math.log10(rng * rng / float((d * d).mean()))


def gain(torch, eng, vol, chunks, bpp):
    n = vol.numel()
    target = int(bpp * n / 8)
    dealt, budgets = eng.compress_to_size(vol, chunks, target, return_plan=True)
    dealt = dealt.clone()
    nchunks = len(budgets)
    per_n = n // nchunks
    hdr = (20 if nchunks > 1 else 14) + 4 * nchunks + 26 * nchunks
    per = max(1, -(-(dealt.numel() - hdr) // nchunks))   # payload bytes a chunk of the uniform container
    uni = eng.compress(vol, chunks, per * 8 / per_n).clone()
    while uni.numel() < dealt.numel():
        per += 1
        uni = eng.compress(vol, chunks, per * 8 / per_n).clone()
    pd, pu = psnr(torch, eng, vol, dealt), psnr(torch, eng, vol, uni)
    b = [int(v) for v in budgets]
    return {"bpp": bpp, "target_bytes": target, "dealt_bytes": dealt.numel(), "uniform_bytes": uni.numel(),
            "uniform_bpp": per * 8 / per_n, "psnr_dealt_db": round(pd, 2), "psnr_uniform_db": round(pu, 2),
            "gain_db": round(pd - pu, 2), "budget_bits_min": min(b), "budget_bits_max": max(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bpp", type=float, default=2.0)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "size_bench.json"))
    args = ap.parse_args()
    import torch
    from sperr_amd.api import SperrHip
    from sperr_amd.synth import turbulence_torch
    eng = SperrHip()
    rec = {"runs": args.runs, "warmup": args.warmup, "bpp": args.bpp, "device": torch.cuda.get_device_name(0), "calls": {},
           "gain": {}}
    for n in [int(s) for s in args.sizes.split(",")]:
        vol = turbulence_torch((n, n, n), "cuda").contiguous()
        for cz in (256, 128):
            if cz > n:
                continue
            chunks = (cz, cz, cz)
            target = int(args.bpp * vol.numel() / 8)
            out = torch.empty(eng.max_compressed_size(vol.shape, chunks, args.bpp), dtype=torch.uint8, device="cuda")
            fns = {"compress_mode1": lambda: eng.compress(vol, chunks, args.bpp, out=out),
                   "compress_to_size": lambda: eng.compress_to_size(vol, chunks, target, out=out),
                   "size_survey": lambda: eng.size_survey(vol, chunks)}
            ms = timed(torch, fns, args.runs, args.warmup)
            r = {k: stats(v) for k, v in ms.items()}
            r["ratio_to_mode1"] = round(r["compress_to_size"]["median"] / r["compress_mode1"]["median"], 3)
            lis = kernel_ms(torch, eng, fns["size_survey"], "k_lis_bits", max(3, args.runs // 3), 1)
            nodes = vol.numel() / 8.0 * 8.0 / 7.0   # (leaf parents and the levels above them)
            r["k_lis_bits"] = stats(lis)
            r["k_lis_bits_bytes"] = int(2 * nodes)
            r["k_lis_bits_fraction_of_hbm_peak"] = round(2 * nodes / (statistics.median(lis) * 1e-3) / HBM_PEAK, 4)
            rec["calls"]["%d^3 in %d^3" % (n, cz)] = r
            print(n, cz, json.dumps(r), flush=True)
    m = 256
    fields = {"turbulence": turbulence_torch((m, m, m), "cuda").contiguous(), "plume": plume_field(torch, m)}
    for name, vol in fields.items():
        rec["gain"][name] = [gain(torch, eng, vol, (64, 64, 64), bpp) for bpp in (0.5, 1.0, 2.0)]
        print(name, json.dumps(rec["gain"][name]), flush=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
