"""CPU: sperr_amd/csrc/fields.h -- what interleaved fields are (the validity rule, the extent, the offset map, the
stacked side's size, the condition of the 16-byte forms) and the LDS slot map of the two kernels of fields.hip -- checked
by tests/cpp/fields_check.cpp, a program of its own built with the address and undefined sanitizers and run directly.
The header is plain C++, so the host compiler builds it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


def test_fields_rule_extent_map_and_lds_slots_under_sanitizers(tmp_path):
    exe = tmp_path / "fields_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "fields_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "fields_check ok" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-3000:]
