"""GPU: the fused finest-level kernels (k_lift_xyz_fwd, lift_xyz_fwd.hip; k_lift_xyz_inv, lift_xyz_inv.hip) with the y and x passes in narrower
windows (lift_window: 4 outputs of a 12-sample window where the workgroup then has a task per thread).

Everything is compared against the CPU oracle, never against the library itself: a compressed container byte for byte
(the forward kernel, and in PWE mode the inverse kernel's brick variant -- doubles into the chunk buffer, no mean --
through the outliers it finds), a decoded volume bit for bit as fp32 and as fp64 (the inverse kernel, IO 1 and 2).

The fused kernels run only for chunks whose transform is dyadic with full-size x, y and z passes first (fuse_xyz,
engine.hip: ShapePlan::schedule.head); every other shape takes the per-axis kernels.  `fused()` below restates that rule, and FUSED / UNFUSED say
for every shape of this file which path it is meant to take: a shape edited off its path fails test_shapes_take_the_path_meant.

The cases are the corners of the passes' task arithmetic: row lengths 2 (too short for these kernels: the other path has
to stay right), 17, 64, 200 and 256 (odd; one segment of 64 samples; a multiple of 4 and 8 but not of 64, so the box
rows are loaded per group; four segments, the box rows through LDS and a task for every thread); slices whose last
tile has 7, 8, 11, 4, 13 and 1 rows (nt < 16, and nt no multiple of the 4 or 8 outputs of a task); odd and even cz; one
chunk and eight chunks in a call, with slices long enough that a tile's slices are dealt to two and to four workgroups
(nseg > 1), the widest rows among them; a box decode (kCrop); a PWE container; a constant chunk beside a normal one;
and chunks with more than 32 bit planes decoded down to the last plane, which keep magnitudes and masks (scheme 0, `wide`)."""
import numpy as np
import pytest

from fields import ramp_field, smooth_field
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def roundtrip(eng, oracle, v, ch, mode, q, tag):
    """compress on the GPU == the oracle's container; both decodes of it == the oracle's; -> the container"""
    want = oracle.comp_3d(v, ch, mode, q)
    got = bytes(eng.compress(cuda(v), ch, q, mode=mode).cpu().numpy())
    assert got == want, (tag, "container differs from the oracle's")
    dev = cuda(np.frombuffer(want, dtype=np.uint8))
    for of in (True, False):
        ref = oracle.decomp_3d(want, of)
        back = eng.decompress(dev, output_float=of).cpu().numpy()
        assert back.shape == ref.shape and back.dtype == ref.dtype, (tag, of)
        assert np.array_equal(bits(back), bits(ref)), (tag, "fp32" if of else "fp64", "decoded volume differs")
    return want


def xforms(n):
    """levels an axis of n samples is halved (num_of_xforms, include/compat/sperr_helper.h)"""
    k = 0
    while n >= 9 and k < 6:
        n -= n // 2
        k += 1
    return k


def fused(ch):
    """fuse_xyz (engine.hip; the plan keeps its answer as schedule.head): a dyadic plan (can_use_dyadic), every axis transformed, 24 staged rows within 6144 samples"""
    xy, z = xforms(min(ch[0], ch[1])), xforms(ch[2])
    return min(ch) >= 9 and 24 * ch[0] <= 6144 and (xy == z or (xy >= 5 and z >= 5))


# chunk dims (x, y, z): cy % 16 = 7, 8, 11, 4, 13, 8; cz odd and even
ROW_CASES = [(2, 23, 20), (17, 24, 19), (64, 43, 33), (200, 36, 40), (256, 29, 21), (256, 40, 50)]
# cz >= 48: two workgroups a tile, cz >= 96: four (launch_lift_xyz)
SHARED_CASES = [(64, 40, 52), (40, 43, 51), (72, 67, 100), (66, 65, 97)]
WIDEST_SHARED = (256, 65, 96)
PWE_CASES = [((64, 43, 33), np.float32), ((200, 36, 40), np.float64), ((256, 29, 21), np.float32)]
BOX_CHUNK, CONST_CHUNK, WIDE_CHUNKS = (64, 40, 52), (64, 43, 33), [(32, 32, 32), (64, 33, 40)]

UNFUSED = [(2, 23, 20)]
FUSED = [c for c in ROW_CASES if c not in UNFUSED] + SHARED_CASES + [WIDEST_SHARED] + [c for c, _ in PWE_CASES] + \
        [BOX_CHUNK, CONST_CHUNK] + WIDE_CHUNKS


def test_shapes_take_the_path_meant():
    assert [c for c in FUSED if not fused(c)] == [] and [c for c in UNFUSED if fused(c)] == []
    assert {c[0] for c in FUSED} >= {17, 64, 200, 256}
    assert any(c[0] == 256 and c[2] >= 96 for c in FUSED) and any(c[2] % 2 for c in FUSED if c[0] == 256)


@pytest.mark.parametrize("ch", ROW_CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_lengths_one_chunk(eng, oracle, ch, dtype):
    v = turbulence((ch[2], ch[1], ch[0]), dtype=dtype)
    roundtrip(eng, oracle, v, ch, 1, 2.0, (ch, dtype.__name__))
    roundtrip(eng, oracle, v, ch, 1, 7.5, (ch, dtype.__name__))


@pytest.mark.parametrize("ch", SHARED_CASES)
def test_one_and_eight_chunks_share_slices(eng, oracle, ch):
    """one chunk, then eight of them in a call"""
    one = smooth_field((ch[2], ch[1], ch[0]), seed=3, passes=1)
    roundtrip(eng, oracle, one, ch, 1, 3.0, (ch, "one chunk"))
    eight = turbulence((2 * ch[2], 2 * ch[1], 2 * ch[0]))
    roundtrip(eng, oracle, eight, ch, 1, 3.0, (ch, "eight chunks"))


def test_widest_rows_shared_by_four_workgroups(eng, oracle):
    """cx = 256: a task for every thread, box rows through LDS, and a tile's slices dealt to four workgroups"""
    ch = WIDEST_SHARED
    roundtrip(eng, oracle, turbulence((ch[2], ch[1], ch[0])), ch, 1, 2.0, (ch, "one chunk"))
    roundtrip(eng, oracle, turbulence((ch[2], ch[1], 2 * ch[0])), ch, 1, 5.0, (ch, "two chunks"))


def test_box_decode(eng, oracle):
    """kCrop: boxes that start and end inside tiles, on odd x, over chunk borders, and a single slice"""
    ch = BOX_CHUNK
    v = turbulence((104, 80, 128))
    c = roundtrip(eng, oracle, v, ch, 1, 4.0, "box")
    dev = cuda(np.frombuffer(c, dtype=np.uint8))
    for of in (True, False):
        full = oracle.decomp_3d(c, of)
        for lo, dims in [((0, 0, 0), (128, 80, 104)), ((3, 5, 7), (40, 30, 41)), ((61, 17, 50), (9, 22, 5)),
                         ((127, 79, 103), (1, 1, 1)), ((1, 33, 51), (126, 13, 1)), ((64, 40, 52), (64, 40, 52))]:
            got = eng.decompress_box(dev, lo, dims, output_float=of).cpu().numpy()
            want = full[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]]
            assert got.shape == want.shape
            assert np.array_equal(bits(got), bits(want)), (lo, dims, of)


@pytest.mark.parametrize("ch,dtype", PWE_CASES)
def test_pwe_container(eng, oracle, ch, dtype):
    """mode 3: the encoder decodes its own coefficients with the inverse kernel's brick variant to find the outliers"""
    v = turbulence((ch[2], 2 * ch[1], ch[0]), dtype=dtype)
    for tol in (1e-2, 1e-4):
        roundtrip(eng, oracle, v, ch, 3, tol, (ch, "pwe", tol))


def test_constant_chunk_beside_a_normal_one(eng, oracle):
    ch = CONST_CHUNK
    v = turbulence((33, 43, 192))
    v[:, :, 64:128] = np.float32(1.25)
    c = roundtrip(eng, oracle, v, ch, 1, 2.0, "constant")
    dev = cuda(np.frombuffer(c, dtype=np.uint8))
    full = oracle.decomp_3d(c, True)
    got = eng.decompress_box(dev, (60, 3, 2), (70, 37, 30)).cpu().numpy()
    assert np.array_equal(bits(got), bits(full[2:32, 3:40, 60:130]))
    roundtrip(eng, oracle, v, ch, 3, 1e-3, "constant, pwe")


def test_all_planes_of_wide_chunks(eng, oracle):
    """more than 32 bit planes, decoded to the last one: the chunk keeps magnitudes and masks (coef_scheme 0, `wide`)"""
    v = smooth_field((32, 32, 64), dtype=np.float64)
    v[:, :, :32] = 0.75
    c = roundtrip(eng, oracle, v, WIDE_CHUNKS[0], 2, 230.0, "psnr 230")
    assert c[20 + 8 + 17 + 17] > 32   # the second chunk has more than 32 bit planes
    w = np.concatenate([smooth_field((40, 33, 64), seed=41, dtype=np.float64), ramp_field((40, 33, 64), dtype=np.float64)], axis=2)
    for rate in (24.0, 40.0, 63.0):
        roundtrip(eng, oracle, w, WIDE_CHUNKS[1], 1, rate, ("rate", rate))
