"""CPU: sperr_amd/csrc/view.h -- what a strided view is (the validity rule, the extent, the index-to-address map and
the cursor the quality kernel walks with) -- checked by tests/cpp/view_check.cpp, a program of its own built with the
address and undefined sanitizers and run directly.  The header is plain C++, so the host compiler builds it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


def test_view_rule_extent_and_map_under_sanitizers(tmp_path):
    exe = tmp_path / "view_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "view_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "view_check ok" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-3000:]
