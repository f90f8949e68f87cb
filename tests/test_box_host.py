"""CPU: the host side of the sub-box decode (include/sperr_hip.h, sperrhip_box_chunks / sperrhip_decomp_3d_box).

Which chunks a box meets follows chunk_volume's segments (a remainder under half a chunk is merged into the
last segment), so it is checked against a brute-force intersection over the oracle's own chunk list.  The
refusals of the host entry point happen before any device is touched."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from sperr_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(api.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sperr_amd", "csrc"), "-j4"])
    return api.load_library()


def brute(oracle, vol, ch, lo, dims):
    out = []
    for i, c in enumerate(oracle.chunk_volume(vol, ch)):
        if all(c[2 * a] < lo[a] + dims[a] and lo[a] < c[2 * a] + c[2 * a + 1] for a in range(3)):
            out.append(i)
    return out


def random_case(rng):
    vol = [rng.choice([1, 2, 3, rng.randint(1, 40), rng.randint(30, 300)]) for _ in range(3)]
    ch = [rng.choice([1, rng.randint(1, 24), rng.randint(8, 64), v, v + rng.randint(0, 5)]) for v in vol]
    kind = rng.randrange(5)
    if kind == 0:     # the whole volume
        lo, dims = [0, 0, 0], list(vol)
    elif kind == 1:   # one voxel
        lo = [rng.randrange(v) for v in vol]
        dims = [1, 1, 1]
    elif kind == 2:   # on the far faces
        dims = [rng.randint(1, v) for v in vol]
        lo = [v - d for v, d in zip(vol, dims)]
    else:
        lo = [rng.randrange(v) for v in vol]
        dims = [rng.randint(1, v - l) for v, l in zip(vol, lo)]
    return vol, ch, lo, dims


def test_box_chunks_matches_brute_force(lib, oracle):
    rng = random.Random(20261016)
    n = 0
    for _ in range(600):
        vol, ch, lo, dims = random_case(rng)
        assert api.box_chunks(lib, vol, ch, lo, dims) == brute(oracle, vol, ch, lo, dims), (vol, ch, lo, dims)
        n += 1
    assert n == 600


@pytest.mark.parametrize("vol,ch,lo,dims", [
    ((300, 40, 70), (256, 32, 32), (255, 0, 0), (2, 40, 70)),      # x: 300 = 256 + 44, 44 < 128: merged
    ((300, 40, 70), (256, 32, 32), (280, 35, 65), (20, 5, 5)),     # inside the merged remainder chunk
    ((400, 50, 70), (256, 32, 32), (255, 31, 63), (2, 2, 2)),      # 400 = 256 + 144: a short last chunk
    ((64, 64, 64), (32, 32, 32), (31, 31, 31), (2, 2, 2)),         # all eight chunks
    ((64, 64, 64), (32, 32, 32), (63, 63, 63), (1, 1, 1)),         # the far corner
    ((10, 10, 10), (16, 16, 16), (3, 4, 5), (1, 1, 1)),            # chunk larger than the volume
])
def test_box_chunks_merged_and_short_remainders(lib, oracle, vol, ch, lo, dims):
    assert api.box_chunks(lib, vol, ch, lo, dims) == brute(oracle, vol, ch, lo, dims)


def test_box_chunks_count_query_and_small_buffer(lib):
    lo, dims, count = (C.c_size_t * 3)(31, 31, 31), (C.c_size_t * 3)(2, 2, 2), C.c_size_t(0)
    assert lib.sperrhip_box_chunks(64, 64, 64, 32, 32, 32, lo, dims, None, 0, C.byref(count)) == 1
    assert count.value == 8
    ids = (C.c_uint32 * 8)(*([0xdead] * 8))
    assert lib.sperrhip_box_chunks(64, 64, 64, 32, 32, 32, lo, dims, ids, 7, C.byref(count)) == 1
    assert list(ids) == [0xdead] * 8, "a buffer that is too small is left alone"
    assert lib.sperrhip_box_chunks(64, 64, 64, 32, 32, 32, lo, dims, ids, 8, C.byref(count)) == 0
    assert list(ids) == list(range(8))


@pytest.mark.parametrize("lo,dims", [
    ((0, 0, 0), (0, 4, 4)), ((0, 0, 0), (4, 0, 4)), ((0, 0, 0), (4, 4, 0)),   # an extent of 0
    ((30, 0, 0), (3, 4, 4)), ((0, 40, 0), (1, 1, 1)), ((0, 0, 20), (1, 1, 5)),   # leaves the volume
    ((32, 0, 0), (1, 1, 1)), ((0, 0, 0), (33, 40, 24)),
    ((2**63, 0, 0), (2**63, 1, 1)),                                            # wraps
])
def test_refusals_without_a_device(lib, oracle, lo, dims):
    vol = np.linspace(0, 1, 32 * 40 * 24, dtype=np.float32).reshape(24, 40, 32)
    stream = oracle.comp_3d(vol, (16, 16, 16), 1, 4.0)
    count = C.c_size_t(12345)
    L, D = (C.c_size_t * 3)(*lo), (C.c_size_t * 3)(*dims)
    assert lib.sperrhip_box_chunks(32, 40, 24, 16, 16, 16, L, D, None, 0, C.byref(count)) == -1
    buf = np.frombuffer(stream, dtype=np.uint8)
    for of in (1, 0):
        dst = C.c_void_p(None)
        assert lib.sperrhip_decomp_3d_box(buf.ctypes.data, buf.size, of, L, D, C.byref(dst)) == -1
        assert dst.value is None, "nothing is written on a refusal"


def test_host_box_refuses_damaged_header_and_busy_dst(lib, oracle):
    vol = np.linspace(0, 1, 16 * 16 * 16, dtype=np.float32).reshape(16, 16, 16)
    stream = bytearray(oracle.comp_3d(vol, (8, 8, 8), 1, 4.0))
    L, D = (C.c_size_t * 3)(0, 0, 0), (C.c_size_t * 3)(4, 4, 4)
    buf = (C.c_uint8 * len(stream)).from_buffer(stream)
    taken = C.c_void_p(1234)
    assert lib.sperrhip_decomp_3d_box(buf, len(stream), 1, L, D, C.byref(taken)) == 1
    assert taken.value == 1234
    for cut in (0, 10, 19, len(stream) - 1):   # shorter than its header / its length table says
        dst = C.c_void_p(None)
        assert lib.sperrhip_decomp_3d_box(buf, cut, 1, L, D, C.byref(dst)) == -1
        assert dst.value is None
    stream[0] = 7   # another version
    dst = C.c_void_p(None)
    assert lib.sperrhip_decomp_3d_box(buf, len(stream), 1, L, D, C.byref(dst)) == -1
    assert dst.value is None
