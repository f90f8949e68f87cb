"""CPU: sperr_amd/csrc/budget.h compiled as host C++ -- a program of its own, tests/cpp/size_check.cpp, under
-fsanitize=address,undefined -- against tests/size_model.py: the deal of every hand-made table at every probed W, budget
by budget and threshold by threshold (the header finds T* by bisection over bit patterns, the model walks a sorted
list: two statements of one rule); the refusal; the container's payload bits; and the header's 128-bit multiply-divide
against the compiler's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import size_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")
TABLES = sm.hand_tables()

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("size_check") / "size_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "size_check.cpp"), "-o", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def bits_of(T):
    return int(np.float64(T).view(np.uint64))


def test_parts_of_the_header(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "size_check ok" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("name", sorted(TABLES))
def test_header_deals_what_the_model_deals(exe, tmp_path, name):
    table = TABLES[name]
    sm.write_table(tmp_path / "table.bin", table)
    ws = sm.probe_budgets(table)
    r = subprocess.run([str(exe), str(tmp_path / "table.bin")] + [str(w) for w in ws], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(ws)
    for W, line in zip(ws, lines):
        head, _, tail = line.partition(":")
        f = head.split()
        assert f[0] == "W" and int(f[1]) == W
        want = sm.deal(table, W)
        if want is None:
            assert int(f[3]) == -1, line
            continue
        budgets, star, nxt = want
        assert int(f[3]) == 0, line
        assert [int(v) for v in tail.split()] == budgets, (W, line, budgets)
        assert int(f[5]) == bits_of(star) and int(f[6]) == (0 if nxt is None else bits_of(nxt)), (W, line, star, nxt)


def test_payload_bits(exe):
    for target, n, nconst in ((0, 1, 0), (44, 1, 0), (45, 1, 0), (1 << 20, 8, 3), (20 + 32 + 26 * 5 + 17 * 3 + 4, 8, 3),
                              (20 + 32 + 26 * 5 + 17 * 3 + 5, 8, 3), (35, 1, 1), (34, 1, 1)):
        r = subprocess.run([str(exe), "payload", str(target), str(n), str(nconst)], capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-2000:]
        want = sm.payload_bits(target, n, nconst)
        assert r.stdout.strip() == ("refused" if want is None else "W %d" % want), (target, n, nconst, r.stdout)
