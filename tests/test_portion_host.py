"""CPU: the host side of portions -- the rule that says how many bytes of a chunk stream a portion keeps
(sperrhip_portion_len, hostc::portion_len), sperr_trunc_3d built on it, and the checks of sperr3d's --pct.

Truncation is byte surgery in the oracle and in the reference (src/SPERR3D_Stream_Tools.cpp:134-226): neither
looks into a chunk stream, so the container here is a header, a length table and random bytes.  Expected values are
the oracle's (oracle.trunc_3d), never the library's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
PCTS = [0, 1, 33, 50, 99, 100, 250]
_sz, _vp = C.c_size_t, C.c_void_p


@pytest.fixture(scope="module")
def lib():
    from sperr_amd import api
    if not os.path.exists(api.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sperr_amd", "csrc"), "-j4"])
    lib = C.CDLL(api.LIB_PATH)
    lib.sperrhip_portion_len.restype = _sz
    lib.sperrhip_portion_len.argtypes = [_sz, C.c_uint]
    lib.sperr_trunc_3d.restype = C.c_int
    lib.sperr_trunc_3d.argtypes = [_vp, _sz, C.c_uint, C.POINTER(_vp), C.POINTER(_sz)]
    return lib


def fabricate(lens, vol=(12, 8, 8), chunk=(4, 4, 4), seed=7):
    """a multi-chunk fp32 container of 3 x 2 x 2 chunks whose streams have the lengths `lens`"""
    assert len(lens) == 12
    head = bytes([0, 0x40 | 0x20 | 0x10]) + np.array(vol, dtype=np.uint32).tobytes() + \
        np.array(chunk, dtype=np.uint16).tobytes() + np.array(lens, dtype=np.uint32).tobytes()
    body = np.random.default_rng(seed).integers(0, 256, size=sum(lens), dtype=np.uint8).tobytes()
    return head + body


@pytest.fixture(scope="module")
def lens():
    rng = np.random.default_rng(11)
    return [1, 63, 64, 65, 100, 6400, 6401] + [int(x) for x in rng.integers(1, 100001, size=5)]


def table(container, n=12):
    return [int(x) for x in np.frombuffer(container, dtype=np.uint32, count=n, offset=20)]


@pytest.mark.parametrize("pct", PCTS)
def test_portion_len_is_the_oracles_length_table(lib, oracle, lens, pct):
    want = table(oracle.trunc_3d(fabricate(lens), pct))
    got = [lib.sperrhip_portion_len(n, pct) for n in lens]
    assert got == want
    if pct in (0, 100, 250):
        assert got == lens
    else:
        assert all(g == n if n <= 64 else 64 <= g < n for g, n in zip(got, lens))


@pytest.mark.parametrize("pct", PCTS)
def test_host_truncation_is_still_the_oracles(lib, oracle, lens, pct):
    c = fabricate(lens)
    buf = np.frombuffer(c, dtype=np.uint8)
    dst, n = _vp(None), _sz(0)
    assert lib.sperr_trunc_3d(buf.ctypes.data, buf.size, pct, C.byref(dst), C.byref(n)) == 0
    got = C.string_at(dst.value, n.value)
    libc = C.CDLL(None)
    libc.free.argtypes = [_vp]
    libc.free(dst)
    want = oracle.trunc_3d(c, pct)
    assert got == want
    assert (got[1] & 0x80) == (0 if pct in (0, 100, 250) else 0x80)


# ---- sperr3d -d --pct P ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tools(lib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cli")])
    return BIN


def run(tools, *args):
    p = subprocess.run([os.path.join(tools, "sperr3d")] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=600)
    return p.returncode, p.stdout + p.stderr


def test_help_lists_the_pct_option(tools):
    rc, out = run(tools, "--help")
    assert rc == 0 and "--pct" in out and "Percentage (1--100)" in out


@pytest.mark.parametrize("args,message", [
    (("s", "-c", "--pct", 40), "requires -d"),
    (("s", "--pct", 40, "--decomp_f", "o"), "requires -d"),
    (("s", "-d", "--decomp_f", "o", "--pct"), "1 required"),
    (("s", "-d", "--decomp_f", "o", "--pct", "half"), "Could not convert"),
    (("s", "-d", "--decomp_f", "o", "--pct", -5), "Could not convert"),
    (("s", "-d", "--decomp_f", "o", "--pct", 2.5), "Could not convert"),
    (("s", "-d", "--decomp_lowres_f", "o", "--pct", 40), "excludes"),
    (("s", "-d", "--decomp_lowres_d", "o", "--pct", 40), "excludes"),
    (("s", "-d", "--decomp_f", "o", "--pct", 40, "--box_origin", 0, 0, 0), "requires --box_dims"),
])
def test_pct_option_checks(tools, args, message):
    rc, out = run(tools, *args)
    assert rc != 0 and message in out


def test_pct_composes_with_box_and_level(tools, tmp_path):
    """the parser lets --pct through with a box and a level; the run then ends at the missing input file"""
    rc, out = run(tools, tmp_path / "none.sperr", "-d", "--decomp_f", tmp_path / "o", "--pct", 40, "--level", 0,
                  "--box_origin", 0, 0, 0, "--box_dims", 1, 1, 1)
    assert rc != 0 and "Cannot read" in out
