"""CPU: the host side of the slice batch calls.  The output bound (sperrhip_max_compressed_size_2d_batch) is nslice
times the single-slice bound, 0 for no slices and 0 when the product does not fit a size_t; the three names are
declared, listed and exported; and without a GPU the two device calls fail loudly (-1) and write nothing."""
import ctypes as C

import numpy as np
import pytest

from sperr_amd import api

_sz = C.c_size_t
NAMES = ("sperrhip_max_compressed_size_2d_batch", "sperrhip_compress_2d_batch_dev",
         "sperrhip_decompress_2d_batch_dev")


@pytest.fixture(scope="module")
def lib():
    lib = api.load_library()
    lib.sperrhip_max_compressed_size_2d.restype = _sz
    lib.sperrhip_max_compressed_size_2d.argtypes = [_sz, _sz, C.c_int, C.c_double]
    return lib


@pytest.mark.parametrize("dims", [(50, 37), (121, 96), (999, 999), (200, 9), (1, 1)])
@pytest.mark.parametrize("mode,q", [(1, 2.0), (1, 40.0), (2, 90.0), (3, 1e-3)])
def test_slice_batch_bound_is_nslice_times_single(lib, dims, mode, q):
    one = lib.sperrhip_max_compressed_size_2d(*dims, mode, q)
    assert one > 0
    for n in (1, 2, 7, 300, 4096):
        assert lib.sperrhip_max_compressed_size_2d_batch(n, *dims, mode, q) == n * one
    assert lib.sperrhip_max_compressed_size_2d_batch(0, *dims, mode, q) == 0


def test_slice_batch_bound_overflow(lib):
    size_max = _sz(-1).value
    one = lib.sperrhip_max_compressed_size_2d(999, 999, 2, 90.0)
    assert lib.sperrhip_max_compressed_size_2d_batch(size_max // one + 1, 999, 999, 2, 90.0) == 0
    assert lib.sperrhip_max_compressed_size_2d_batch(size_max, 999, 999, 2, 90.0) == 0
    assert lib.sperrhip_max_compressed_size_2d_batch(size_max // one, 999, 999, 2, 90.0) == (size_max // one) * one


def test_slice_batch_names_are_listed_and_exported(lib):
    for name in NAMES:
        assert name in api.EXPORTS
        assert hasattr(lib, name), f"{name} is not exported by the library"


def test_slice_batch_without_a_gpu_fails_loudly(lib):
    """No CPU path behind the device calls: -1, the offsets and both buffers as they were."""
    import torch
    if torch.cuda.is_available():
        return
    n, dy, dx = 3, 20, 24
    src = np.zeros((n, dy, dx), dtype=np.float32)
    dst = np.full(lib.sperrhip_max_compressed_size_2d_batch(n, dx, dy, 1, 2.0), 0xA5, dtype=np.uint8)
    offs = (_sz * (n + 1))(*([77] * (n + 1)))
    rtn = lib.sperrhip_compress_2d_batch_dev(src.ctypes.data, 1, n, dx, dy, 1, 2.0, 0, dst.ctypes.data, dst.size, offs,
                                             None)
    assert rtn == -1 and list(offs) == [77] * (n + 1) and bool((dst == 0xA5).all())
    streams = np.zeros(3 * 40, dtype=np.uint8)
    o = (_sz * (n + 1))(0, 40, 80, 120)
    out = np.full((n, dy, dx), 7.5, dtype=np.float32)
    for hdr in (0, 1):
        rtn = lib.sperrhip_decompress_2d_batch_dev(streams.ctypes.data, o, n, hdr, 1, dx, dy, out.ctypes.data,
                                                   out.nbytes, None)
        assert rtn == -1 and bool((out == 7.5).all())
