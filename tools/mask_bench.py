#!/usr/bin/env python3
"""mask_bench.py -- what missing values cost: a 512^3 fp32 turbulence volume in 256^3 chunks at 2 bpp, with a ball of
NaNs of about a third of the samples (a stream of toggles) and with NaNs of density 0.1 (a stream of bits).

  (a) mask_make with the fill, and mask_apply, in ms and as bytes moved over time -- two reads and one write of the
      volume and the stream for the first, the stream and the stores at the missing samples for the second.  Beside
      them the torch formulation of the same work in the same process, which is the yardstick: isnan -> where with the
      midrange of the valid samples (amin and amax of a where with +-inf at the missing ones: no compaction, no
      host wait) -> a bit-packing; and an unpacking -> masked_fill_
  (b) compress_masked against compress of the volume that already is in-filled: the difference is the feature's cost
  (c) decompress_masked against decompress

Every figure is the median (and min ... max) of --runs calls after --warmup, each timed with events on the current
stream around the call alone; the two sides of every comparison alternate run by run.

  python tools/mask_bench.py [--runs 15] [--warmup 3] [--n 512] [--out profiles/mask_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_sz = C.c_size_t
BPP = 2.0


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def timed(torch, fns, runs, warmup):
    """{name: [ms]} of the calls in fns, alternating run by run so that both sides of a comparison see the same
    clocks and the same neighbours"""
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


def torch_make(torch, v, weights):
    """the torch formulation of mask_make with the fill: (packed bits, in-filled volume)"""
    m = torch.isnan(v)
    lo = torch.where(m, float("inf"), v).amin()      # (no compaction, no host wait: v[~m] would need both)
    hi = torch.where(m, float("-inf"), v).amax()
    f = (0.5 * lo.double() + 0.5 * hi.double()).float()
    filled = torch.where(m, f, v)
    packed = (m.view(-1, 8).to(torch.uint8) * weights).sum(dim=1, dtype=torch.uint8)
    return packed, filled


def torch_apply(torch, out, packed, shifts, value):
    """... and of mask_apply: the packed bits back to a bool tensor, then masked_fill_"""
    m = ((packed[:, None] >> shifts) & 1).view(torch.bool).view(out.shape)
    return out.masked_fill_(m, value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_bench.json"))
    args = ap.parse_args()

    import torch
    from sperr_amd.api import SperrHip
    from sperr_amd.synth import turbulence_torch
    eng = SperrHip()
    n = args.n
    chunks = (min(256, n),) * 3
    base = turbulence_torch((n, n, n), "cuda", dtype=torch.float32)
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - n / 2
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    radius = n * (1.0 / (4.0 * torch.pi)) ** (1.0 / 3.0)      # 4/3 pi r^3 = n^3 / 3
    masks = {"ball": r2 <= radius * radius,
             "density_0.1": torch.rand((n, n, n), device="cuda", generator=torch.Generator("cuda").manual_seed(7)) < 0.1}
    del r2
    weights = (1 << torch.arange(8, device="cuda")).to(torch.uint8)
    shifts = torch.arange(8, device="cuda", dtype=torch.uint8)
    nan = float("nan")
    result = {"volume": [n, n, n], "dtype": "float32", "chunks": list(chunks), "bpp": BPP, "runs": args.runs,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "cases": {}}
    nsamp = n ** 3
    for name, m in masks.items():
        v = torch.where(m, torch.full_like(base, nan), base)
        nmiss = int(m.sum())
        filled = torch.empty_like(v)
        buf = torch.empty(eng.mask_max_size(nsamp), dtype=torch.uint8, device="cuda")
        mlen, cnt = _sz(0), _sz(0)

        def make():
            rtn = eng.lib.sperrhip_mask_make_dev(v.data_ptr(), 1, nsamp, 1, 0.0, filled.data_ptr(), buf.data_ptr(),
                                                 buf.numel(), C.byref(mlen), C.byref(cnt), eng._stream())
            assert rtn == 0
        make()
        stream = buf[:mlen.value]
        _, _, kind = eng.mask_parse(stream)
        packed, tfilled = torch_make(torch, v, weights)
        assert cnt.value == nmiss and torch.equal(filled, tfilled), "the two formulations fill differently"
        assert torch.equal(eng.mask_bits(stream).view(m.shape), m)
        del tfilled
        out = torch.zeros_like(v)
        case = {"missing": nmiss, "fraction": round(nmiss / nsamp, 4), "kind": kind, "mask_bytes": mlen.value}
        ms = timed(torch, {"lib": make, "torch": lambda: torch_make(torch, v, weights)}, args.runs, args.warmup)
        moved = 3 * 4 * nsamp + mlen.value
        case["mask_make_fill"] = dict(stats(ms["lib"]), bytes_moved=moved,
                                      GBps=round(moved / statistics.median(ms["lib"]) / 1e6, 1))
        case["torch_make_fill"] = stats(ms["torch"])
        ms = timed(torch, {"lib": lambda: eng.mask_apply(out, stream, nan),
                           "torch": lambda: torch_apply(torch, out, packed, shifts, nan)}, args.runs, args.warmup)
        moved = mlen.value + 4 * nmiss
        case["mask_apply"] = dict(stats(ms["lib"]), bytes_moved=moved,
                                  GBps=round(moved / statistics.median(ms["lib"]) / 1e6, 1))
        case["torch_apply"] = stats(ms["torch"])
        del packed, out
        # (b) and (c): the masked calls against the parent's own calls on the in-filled volume
        container, stream2 = eng.compress_masked(v, chunks, BPP)
        dense = eng.compress(filled, chunks, BPP)
        assert torch.equal(container, dense) and torch.equal(stream2, stream)
        case["container_bytes"] = container.numel()
        ms = timed(torch, {"masked": lambda: eng.compress_masked(v, chunks, BPP),
                           "dense": lambda: eng.compress(filled, chunks, BPP)}, args.runs, args.warmup)
        case["compress_masked"], case["compress_infilled"] = stats(ms["masked"]), stats(ms["dense"])
        back = torch.empty_like(v)
        ms = timed(torch, {"masked": lambda: eng.decompress_masked(container, stream, nan, out=back),
                           "dense": lambda: eng.decompress(container, out=back, shape_zyx=(n, n, n))},
                   args.runs, args.warmup)
        case["decompress_masked"], case["decompress"] = stats(ms["masked"]), stats(ms["dense"])
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        del v, filled, back, container, dense
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    eng.release()


if __name__ == "__main__":
    main()
