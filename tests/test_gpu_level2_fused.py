"""GPU: the second transform level as one launch each way (k_lift2_fwd, lift_xyz_fwd.hip; k_lift2_inv<SG>, lift_xyz_inv.hip; plan_level2,
engine.hip) against the three per-axis passes it replaces.

Every case runs with the new kernels on and with SPERR_HIP_XYZ_LEVEL2=0: the switch is read whenever a chunk shape's
plan is made, and release() drops the plans.  Both containers have to equal the CPU oracle's byte for byte -- so they equal
each other -- and both decodes of it, as fp32 and as fp64, the oracle's bit for bit.  The kernel profile says which path
ran: on a FUSED shape the new kernels appear with the switch on and k_lift_axis<.., 0> runs three launches fewer per
level-2 launch, in each direction; with the switch off, and on an UNFUSED shape either way, no level-2 kernel runs and
the per-axis launch counts are the same.

"On" is SPERR_HIP_XYZ_LEVEL2=2 here: the launch wherever it fits.  By default (=1) both directions take it only where
the level-2 region has at least 96 samples along every axis (plan_level2, engine.hip: where it was measured to gain); =2
drops that floor, so that the kernels meet every shape of this file.  The default is checked as well: the same
containers and decodes, the new kernels exactly where `by_default()` says.

`level2()` restates level2_fits (engine.hip, one of the rules behind ShapePlan::schedule): a dyadic plan whose finest level is fused (test_gpu_xyz_passes.fused), a second level
on every axis -- an axis of n samples is halved while n >= 9, so the level-2 region has at least 9 samples a side and a
chunk 16 samples a side has no second level at all --, and region rows of at most 128 samples.

Shapes (z, y, x), for where the kernels can go wrong:
  (16, 16, 16)     one level only: nothing to fuse (UNFUSED)
  (19, 24, 17)     odd region lengths on every axis, (10, 12, 9): five pairs along z, shorter than the run-up of six
  (33, 43, 64)     a region of 22 rows: a full tile and a partial one; also as a batch of three chunks with a constant
                   one, as fp64 input, and under decompress_box with windows that cross the region
  (50, 40, 256)    region rows of 128 samples, the widest allowed: every lane of the inverse kernel's box loads in use
  (192, 129, 130)  a region 96 deep in five tiles: the segment rule deals a tile's slices to four workgroups
                   (cz / (2 nseg) >= 24); the smallest dyadic shape that deep (five levels need 129 samples)
  (192, 192, 192)  the smallest cube above the default's floor: the one shape here that takes the launch by default
  (20, 20, 512)    rows of 512 samples: the finest level is not fused, so neither is the second (UNFUSED)"""
import os

import numpy as np
import pytest

from fields import smooth_field
from sperr_amd.synth import turbulence
from test_gpu_xyz_passes import bits, cuda, fused, xforms

pytestmark = pytest.mark.gpu
SWITCH = "SPERR_HIP_XYZ_LEVEL2"

FUSED = [(19, 24, 17), (33, 43, 64), (50, 40, 256), (192, 129, 130), (192, 192, 192)]
UNFUSED = [(16, 16, 16), (20, 20, 512)]
DEEP = (192, 129, 130)


def level2(zyx):
    ch = (zyx[2], zyx[1], zyx[0])
    region = [n - n // 2 for n in ch]
    return fused(ch) and min(xforms(n) for n in ch) >= 2 and min(region) >= 9 and region[0] <= 128


def by_default(zyx):
    """plan_level2: the default's floor on top of level2()"""
    return level2(zyx) and min(n - n // 2 for n in zyx) >= 96


def segments(zyx, nchunks=1):
    """launch_lift_xyz's rule for the level-2 launch of `nchunks` chunks"""
    region = [n - n // 2 for n in zyx]
    ntile, nseg = (region[1] + 15) // 16, 1
    while nseg < 4 and ntile * nchunks * nseg < 512 and region[0] // (2 * nseg) >= 24:
        nseg *= 2
    return nseg


def test_shapes_take_the_path_meant():
    assert [s for s in FUSED if not level2(s)] == [] and [s for s in UNFUSED if level2(s)] == []
    assert xforms(16) == 1 and not fused((512, 20, 20))
    assert segments(DEEP) == 4 and all(segments(s) == 1 for s in FUSED if s[0] < 192)
    assert [s for s in FUSED if by_default(s)] == [(192, 192, 192)]   # (both sides of the default's floor)
    assert any(s[2] - s[2] // 2 == 128 for s in FUSED) and any((s[2] - s[2] // 2) % 2 for s in FUSED)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    before = os.environ.get(SWITCH)
    yield e
    if before is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = before
    e.release()


def switch(eng, on):
    """True: the new kernels wherever they apply (2); False: the three passes (0); None: the default (1)"""
    os.environ[SWITCH] = "1" if on is None else "2" if on else "0"
    eng.release()   # (the plans go: the next call makes them again and reads the switch)


def launched(eng, fn):
    """(what fn returns, {kernel name: launches})"""
    import torch
    torch.cuda.synchronize()
    eng.profile(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)


def count(rep, name):
    return sum(n for k, n in rep.items() if name in k)


def both_paths(eng, oracle, v, ch, q, tag, want_fused):
    """compress and decode with the switch on and off; everything against the oracle; the launches as the path says"""
    want = oracle.comp_3d(v, ch, 1, q)
    refs = {of: oracle.decomp_3d(want, of) for of in (True, False)}
    dev = cuda(np.frombuffer(want, dtype=np.uint8))
    reps = {}
    for on in (True, False):
        switch(eng, on)
        got, enc = launched(eng, lambda: bytes(eng.compress(cuda(v), ch, q).cpu().numpy()))
        assert got == want, (tag, on, "container differs from the oracle's")
        dec = {}
        for of in (True, False):
            back, dec[of] = launched(eng, lambda: eng.decompress(dev, output_float=of).cpu().numpy())
            assert back.shape == refs[of].shape and back.dtype == refs[of].dtype, (tag, on, of)
            assert np.array_equal(bits(back), bits(refs[of])), (tag, on, "fp32" if of else "fp64", "decoded volume differs")
        reps[on] = (enc, dec)
    (enc1, dec1), (enc0, dec0) = reps[True], reps[False]
    print(tag, "forward on/off:", {k: n for k, n in enc1.items() if "lift" in k}, {k: n for k, n in enc0.items() if "lift" in k})
    print(tag, "inverse on/off:", {k: n for k, n in dec1[True].items() if "lift" in k}, {k: n for k, n in dec0[True].items() if "lift" in k})
    assert count(enc0, "k_lift2_") == 0 and all(count(dec0[of], "k_lift2_") == 0 for of in dec0), (tag, "switch off", enc0, dec0)
    nf = count(enc1, "k_lift2_fwd")
    assert (nf >= 1) == want_fused, (tag, enc1)
    assert count(enc0, "k_lift_axis<true, 0>") - count(enc1, "k_lift_axis<true, 0>") == 3 * nf, (tag, enc1, enc0)
    for of in (True, False):
        ni = count(dec1[of], "k_lift2_inv")
        assert (ni >= 1) == want_fused, (tag, of, dec1[of])
        assert count(dec0[of], "k_lift_axis<false, 0>") - count(dec1[of], "k_lift_axis<false, 0>") == 3 * ni, (tag, of, dec1[of], dec0[of])
    # the default: the launches where the floor allows
    switch(eng, None)
    zyx = (ch[2], ch[1], ch[0])
    got, enc = launched(eng, lambda: bytes(eng.compress(cuda(v), ch, q).cpu().numpy()))
    assert got == want and count(enc, "k_lift2_fwd") == (nf if by_default(zyx) else 0), (tag, "default", enc)
    for of in (True, False):
        back, rep = launched(eng, lambda: eng.decompress(dev, output_float=of).cpu().numpy())
        assert np.array_equal(bits(back), bits(refs[of])), (tag, "default", of)
        assert (count(rep, "k_lift2_inv") >= 1) == (want_fused and by_default(zyx)), (tag, "default", of, rep)
    return want


@pytest.mark.parametrize("shape", FUSED + UNFUSED)
def test_one_chunk_both_paths(eng, oracle, shape):
    v = smooth_field(shape, seed=7, passes=1) if shape[0] >= 192 else turbulence(shape)
    both_paths(eng, oracle, v, (shape[2], shape[1], shape[0]), 2.0, shape, level2(shape))


def test_three_chunks_one_constant(eng, oracle):
    v = turbulence((33, 43, 192))
    v[:, :, 64:128] = np.float32(-3.5)
    both_paths(eng, oracle, v, (64, 43, 33), 3.0, "three chunks", True)


def test_fp64_input(eng, oracle):
    v = turbulence((33, 43, 64), dtype=np.float64)
    both_paths(eng, oracle, v, (64, 43, 33), 7.5, "fp64", True)


def test_box_decode_across_the_region(eng, oracle):
    """windows that cross the level-2 region (32, 22, 17 samples along x, y, z) of chunks of (33, 43, 64)"""
    v = turbulence((33, 86, 128))
    c = oracle.comp_3d(v, (64, 43, 33), 1, 4.0)
    dev = cuda(np.frombuffer(c, dtype=np.uint8))
    full = {of: oracle.decomp_3d(c, of) for of in (True, False)}
    for on in (True, False):
        switch(eng, on)
        for of in (True, False):
            for lo, dims in [((20, 15, 10), (30, 20, 15)), ((31, 21, 16), (2, 2, 2)), ((50, 30, 0), (40, 30, 33)), ((0, 0, 0), (128, 86, 33))]:
                got, rep = launched(eng, lambda: eng.decompress_box(dev, lo, dims, output_float=of).cpu().numpy())
                wanted = full[of][lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]]
                assert got.shape == wanted.shape and np.array_equal(bits(got), bits(wanted)), (on, of, lo, dims)
                assert (count(rep, "k_lift2_inv") >= 1) == on, (on, rep)
    switch(eng, None)
