"""GPU: k_emit_pixels (speck_enc.hip) -- the kernel that writes the LIP-scan and refinement bits of every coded plane --
on the shapes at which what a thread holds can go wrong, every container byte for byte against the CPU oracle's.

The 32-bit pass holds its 16 magnitudes as plane masks (pix_planes.h: transposed once, two 16-bit planes a register),
takes "msb above / at the plane" from a recurrence down the planes instead of the msb bytes, and expands the LIP tokens
with their signs through a nibble table; the 64-bit pass takes the msb from the magnitude as well.  So: a thread that
straddles the end of the chunk (zero-filled magnitudes), several tiles, budget cuts inside LIP and refinement passes on
and off word boundaries, refinement down to plane 0 with bit 31 set (both halves of the packed planes), samples that
are exactly zero (msb -1, dead and half dead threads), the 64-bit retry behind a 32-bit pass, the modes without a budget,
and the 2D forest through the same kernel."""
import os

import numpy as np
import pytest

from fields import ramp_field, smooth_field

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

BUDGET_RATES = [0.3, 0.47, 0.71, 1.0, 1.37, 1.9, 2.0, 2.6, 3.3, 4.1, 5.2, 6.0]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    return SperrHip()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _zeros(frac, seed):
    """48^3 with `frac` per cent of the samples exactly zero (as _sparse in test_gpu_fused_head.py)"""
    v = smooth_field((48, 48, 48), seed=seed, passes=2)
    v[np.abs(v) < np.float32(np.percentile(np.abs(v), frac))] = 0
    assert abs(float((v == 0).mean()) - frac / 100.0) < 0.02
    return v


def _wide_retry_64():
    return np.concatenate([smooth_field((64, 64, 64), seed=41), ramp_field((64, 64, 64)),
                           smooth_field((64, 64, 64), seed=42)], axis=0)


# name -> (field (z, y, x), chunk dims xyz, [(mode, quality)])
CASES_3D = {
    # 4913 samples: a partial second tile, one thread with samples on both sides of the end
    "partial_tile_17": (lambda: np.fromfile(os.path.join(GOLD, "wmag17.f32"), dtype=np.float32).reshape(17, 17, 17),
                        (17, 17, 17), [(1, 0.5), (1, 2.0), (1, 4.0), (1, 24.0)]),
    "flat_64x64x9": (lambda: smooth_field((9, 64, 64)), (64, 64, 9), [(1, 2.0), (1, 6.0)]),
    "odd_50x37x19": (lambda: smooth_field((19, 37, 50)), (50, 37, 19), [(1, 2.0), (1, 6.0)]),
    "budget_cut_48": (lambda: smooth_field((48, 48, 48)), (48, 48, 48), [(1, r) for r in BUDGET_RATES]),
    "every_plane_smooth_32": (lambda: smooth_field((32, 32, 32)), (32, 32, 32), [(1, 24.0)]),
    "every_plane_ramp_32": (lambda: ramp_field((32, 32, 32)), (32, 32, 32), [(1, 24.0)]),
    "zeros_60": (lambda: _zeros(60, 81), (48, 48, 48), [(1, 2.0), (1, 8.0)]),
    "zeros_85": (lambda: _zeros(85, 82), (48, 48, 48), [(1, 2.0), (1, 8.0)]),
    "wide_retry_64": (_wide_retry_64, (64, 64, 64), [(1, 24.0), (1, 40.0)]),
    "other_modes_f64": (lambda: smooth_field((24, 40, 40), dtype=np.float64), (40, 40, 24), [(2, 100.0), (3, 1e-9)]),
}


@pytest.mark.parametrize("name", list(CASES_3D))
def test_containers_equal_the_oracle(eng, oracle, name):
    field, chunks, runs = CASES_3D[name]
    vol = field()
    for mode, q in runs:
        want = oracle.comp_3d(vol, chunks, mode, q)
        got = bytes(eng.compress(cuda(vol), chunks, q, mode=mode).cpu().numpy())
        print(name, mode, q, "container bytes", len(got), "oracle's", len(want))
        assert got == want, (name, mode, q, "container differs from the oracle's")


def test_every_plane_cases_reach_plane_0_with_bit_31(eng, oracle):
    """what the two `every_plane` cases are for, checked on the coder's own input: at 24 bits per sample a 32^3 chunk is
    coded down to plane 0 inside the budget, from a top plane of 31 where the quantiser's largest magnitude has bit 31
    set -- a SPECK stream of quantised magnitudes that do, through the same kernel, against the oracle"""
    rng = np.random.RandomState(5)
    coef = (rng.randint(0, 1 << 16, size=(32, 32, 32)).astype(np.uint64) << np.uint64(16)) | \
        rng.randint(0, 1 << 16, size=(32, 32, 32)).astype(np.uint64)
    coef >>= rng.randint(0, 33, size=coef.shape).astype(np.uint64)   # every msb from -1 to 31
    coef[0, 0, 0] = 0xFFFFFFFF
    coef[31, 31, 31] = 0x80000000
    coef[5, 6, 7] = 0x80000001
    sign = np.frombuffer(rng.bytes(8 * ((coef.size + 63) // 64)), dtype=np.uint64).copy()
    for budget in (0, 100001, 500000):   # all 32 planes; cuts inside the lower planes, off a word boundary and on one
        want = oracle.speck3d_encode(coef, sign, budget)
        got = eng.speck3d_encode(cuda(coef.astype(np.uint32).view(np.int32)), cuda(sign.view(np.int64)), budget)
        assert got[:9] == want[:9]
        assert got == want, budget
    assert want[0] == 32, "the stream's plane count: bit 31 is set"


SLICES = {
    "slice_37x50": lambda: smooth_field((1, 37, 50))[0],
    "slice_crop_200": lambda: np.ascontiguousarray(
        np.fromfile(os.path.join(GOLD, "img999.f32"), dtype=np.float32).reshape(999, 999)[200:400, 300:500]),
}


@pytest.mark.parametrize("name", list(SLICES))
def test_slices_equal_the_oracle(eng, oracle, name):
    img = SLICES[name]()
    for mode, q in [(1, 2.0), (2, 90.0)]:
        want = oracle.comp_2d(img, mode, q, False)
        got = bytes(eng.compress_2d(cuda(img), q, mode=mode, header=False).cpu().numpy())
        assert got == want, (name, mode, q, "2D stream differs from the oracle's")
