"""CPU: sperr_amd/csrc/poison_env.h -- the parser of SPERR_HIP_POISON, the switch that fills the engine's workspaces
before a call carves them (tests/test_gpu_poison.py runs every device call under it) -- checked by
tests/cpp/poison_env_check.cpp, a program of its own built with the address and undefined sanitizers and run directly.
The header is plain C++, so the host compiler builds it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


def test_poison_switch_parser_under_sanitizers(tmp_path):
    exe = tmp_path / "poison_env_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "poison_env_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k != "SPERR_HIP_POISON"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "poison_env_check ok" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-3000:]
