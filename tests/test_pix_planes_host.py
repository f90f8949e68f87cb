"""CPU: the per-thread arithmetic of k_emit_pixels (sperr_amd/csrc/pix_planes.h) -- the 16-sample transpose into plane
masks, the msb recurrence down the planes, the nibble tables for pext and for the LIP tokens with their signs -- compiled
into tests/cpp/pix_planes_check.cpp, a program of its own under the address and undefined sanitizers, and compared there
bit for bit with the per-sample definitions the kernel used before (bit-sliced msb + 1 through its seven-mask comparison,
bit pl of a magnitude by a shift, the one-sign-per-turn loop)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("pix_planes_check") / "pix_planes_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "sperr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pix_planes_check.cpp"), "-o", str(path)])
    return path


def run(exe, what):
    p = subprocess.run([str(exe), what], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-2000:] + p.stderr[-2000:]


def test_transpose_gives_plane_masks(exe):
    """C[pl] has bit k set exactly when bit pl of sample k is set: random magnitudes of every width, all zeros, all ones,
    single bits at planes 0, 15, 16 and 31, one sample with bit 31 among zeros"""
    run(exe, "transpose")


def test_msb_recurrence_equals_the_bit_sliced_comparison(exe):
    """for p = 31 .. 0: the samples whose msb is above / at p and bit p of the magnitudes, zero magnitudes (msb -1) among
    them, against above_equal on msb + 1 and the per-sample shifts"""
    run(exe, "recurrence")


def test_sign_expansion_equals_the_loop(exe):
    """all 256 (token nibble, sign nibble) entries; every 16-bit token word with 64 random sign words; 10^6 random
    (tok, sgn, nl <= 16); value and length -- and the 16-bit pext in front of it against a loop"""
    run(exe, "signs")
