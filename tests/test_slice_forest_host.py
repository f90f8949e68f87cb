"""CPU: no slice has a forest that k_lis_mx cannot decode.  A slice is decoded on the 2D coder's forest
(spk::build_tree(x, y, 1, twoD), the plan of key (x, y, 0)) by k_lis_mx, the only list kernel with the type-I phase:
there is no other 2D decoder to fall back to.  tests/cpp/slice_forest_check.cpp builds the forest of every shape
below and checks what use_mixed() and use_tables() (engine.hip, the rules behind ShapePlan::dec) test: classes exist (at most 254, or build_classes
gives up and leaves none), at most 48 roots and 352 grids, a column entry per class, and never `allRegular`.
DESIGN.md section 4c argues why these counts stay bounded as the extents grow; this pins the finite part."""
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shapes():
    s = set()
    for x in range(1, 65):                      # every small slice
        for y in range(1, 65):
            s.add((x, y))
    edge = sorted({v for k in range(13) for v in (2 ** k - 1, 2 ** k, 2 ** k + 1) if v >= 1})
    side = sorted(set(edge) | {1, 2, 3, 7, 999})
    for x in edge:                              # around the powers of two, with each other and with 1, 2, 3, 7, 999
        for y in side:
            s.add((x, y))
            s.add((y, x))
    rng = random.Random(20240607)
    for _ in range(160):                        # a fixed random sample up to 4096 x 4096
        s.add((rng.randint(1, 4096), rng.randint(1, 4096)))
    for _ in range(160):                        # (log-uniform: the small and the lopsided ones too)
        s.add((int(2 ** rng.uniform(0, 12)), int(2 ** rng.uniform(0, 12))))
    # extreme aspect ratios, up to the longest extent a chunk can have
    for long_ in (65535, 65534, 32769, 32768, 32767, 40000):
        for short in (1, 2, 3, 8, 9, 17):
            s.add((long_, short))
            s.add((short, long_))
    return sorted(s, key=lambda d: -d[0] * d[1])   # (the big ones first: the threads end together)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("slice_forest_check") / "slice_forest_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
                           "-I", os.path.join(ROOT, "sperr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "slice_forest_check.cpp"), "-o", str(path)])
    return path


def test_every_slice_forest_fits_the_mixed_list_kernel(exe, tmp_path):
    shapes = _shapes()
    assert len(shapes) > 5000 and max(x * y for x, y in shapes) <= 4097 * 4097
    (tmp_path / "shapes.txt").write_text("".join(f"{x} {y}\n" for x, y in shapes))
    nthreads = max(1, min(16, os.cpu_count() or 1))
    p = subprocess.run([str(exe), str(tmp_path / "shapes.txt"), str(nthreads)], capture_output=True, text=True,
                       timeout=1200)
    print(p.stdout[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    m = re.search(r"shapes (\d+) failed (\d+) max_roots (\d+) max_grids (\d+) max_cls (\d+)", p.stdout)
    assert m, p.stdout[-2000:]
    n, failed, roots, grids, cls = map(int, m.groups())
    assert n == len(shapes) and failed == 0
    # the bounds of DESIGN.md section 4c: 1 + 3 * (at most 6 transform levels) roots, each with at most 16 set depths
    assert roots <= 19 and grids <= 19 * 16 and 1 <= cls <= 254
