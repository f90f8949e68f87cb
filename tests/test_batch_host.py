"""CPU: the output bound of a batch compression (sperrhip_max_compressed_size_batch) is nvol times the
single-volume bound, and 0 when that product does not fit a size_t.  Host only: no device is touched."""
import ctypes as C

import pytest

from sperr_amd import api


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


@pytest.mark.parametrize("dims,chunks", [((40, 48, 56), (32, 32, 32)), ((24, 20, 16), (64, 64, 64)),
                                         ((12, 10, 9), (32, 32, 32)), ((256, 256, 256), (128, 128, 256))])
@pytest.mark.parametrize("mode,q", [(1, 2.0), (1, 40.0), (2, 80.0), (3, 1e-3)])
def test_batch_bound_is_nvol_times_single(lib, dims, chunks, mode, q):
    one = lib.sperrhip_max_compressed_size(*dims, *chunks, mode, q)
    assert one > 0
    for nvol in (1, 2, 7, 300, 4096):
        assert lib.sperrhip_max_compressed_size_batch(nvol, *dims, *chunks, mode, q) == nvol * one
    assert lib.sperrhip_max_compressed_size_batch(0, *dims, *chunks, mode, q) == 0


def test_batch_bound_overflow(lib):
    size_max = C.c_size_t(-1).value
    one = lib.sperrhip_max_compressed_size(40, 48, 56, 32, 32, 32, 1, 2.0)
    n = size_max // one + 1
    assert lib.sperrhip_max_compressed_size_batch(n, 40, 48, 56, 32, 32, 32, 1, 2.0) == 0
    assert lib.sperrhip_max_compressed_size_batch(size_max, 40, 48, 56, 32, 32, 32, 1, 2.0) == 0
    assert lib.sperrhip_max_compressed_size_batch(size_max // one, 40, 48, 56, 32, 32, 32, 1, 2.0) == \
        (size_max // one) * one
