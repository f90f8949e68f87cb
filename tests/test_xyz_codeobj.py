"""CPU (hipcc cross-compiles gfx950 here): registers, spills and scratch of the fused finest-level kernels
(k_lift_xyz_fwd in sperr_amd/csrc/lift_xyz_fwd.hip, k_lift_xyz_inv in lift_xyz_inv.hip and, its crop variants,
lift_xyz_inv_crop.hip), read from the code object metadata of the ISA the compiler emits with the Makefile's flags.  The
kernels judged are those of the five units that were one file, xform.hip, when the figures below were taken: the
conditioner and quantiser (xform.hip today) and the lifting units.

Both kernels run one workgroup of 1024 threads per compute unit: 128 VGPRs a thread, not one more.  The forward kernel fits
them.  The inverse kernel does not -- six z pipelines of four fp64 values per thread plus a window of the y / x pass -- and
what it spills decides whether a reload lands inside the slice loop, where `s_waitcnt vmcnt(0)` behind a scratch load
waits for every prefetch and store in flight.  The figures before the passes took 12-sample windows
(lift_window) and the x pass wrote the volume itself were 44 / 52 spilled VGPRs and 100 / 108 bytes of scratch for
<1, true, false> / <2, true, false>, the instantiations the benchmark runs; the ceilings below are what that change
reached, so a later one cannot give it back silently.  No other kernel of these units may use more scratch than it did then."""
import concurrent.futures
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")
# the units with the fused second level's kernels (test_level2_codeobj.py compiles only these) and all the lifting units
LIFT2_UNITS = ["lift_xyz_fwd.hip", "lift_xyz_inv.hip"]
LIFT_UNITS = ["lift_axis.hip", "lift_xyz_inv_crop.hip"] + LIFT2_UNITS
UNITS = ["xform.hip"] + LIFT_UNITS
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-value", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# before the change: spilled VGPRs, bytes of scratch of the instantiations the benchmark runs (IO = 1, 2)
PARENT = {1: (44, 100), 2: (52, 108)}
# what the change reached (the same, pinned)
REACHED = {1: (16, 52), 2: (22, 60)}
# bytes of scratch of every kernel of the units that had any before the change; all others had none
SCRATCH_BEFORE = {
    "k_lift_axisILb0ELi1ELb1E": 40, "k_lift_axisILb0ELi2ELb1E": 40,
    "k_lift_xyz_invILi1ELb0ELb0E": 108, "k_lift_xyz_invILi2ELb0ELb0E": 108,
    "k_lift_xyz_invILi1ELb1ELb0E": 100, "k_lift_xyz_invILi2ELb1ELb0E": 108,
    "k_lift_xyz_invILi1ELb0ELb1E": 108, "k_lift_xyz_invILi2ELb0ELb1E": 108,
    "k_lift_xyz_invILi1ELb1ELb1E": 116, "k_lift_xyz_invILi2ELb1ELb1E": 116,
}


def kernel_meta(s_text):
    """{kernel symbol: {key: int}} from the code object metadata at the end of the ISA file"""
    meta = {}
    for m in re.finditer(r"^\s+- \.agpr_count:.*?(?=^\s+- \.agpr_count:|\Z)", s_text, flags=re.S | re.M):
        blk = m.group(0)
        nm = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[nm] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    return meta


def units_meta(units, tmp_dir):
    """kernel_meta of the union of `units`, compiled side by side; a kernel lives in one unit"""
    def one(unit):
        s_path = os.path.join(str(tmp_dir), unit[:-4] + ".s")
        r = subprocess.run(["hipcc", *FLAGS, "-S", os.path.join(CSRC, unit), "-o", s_path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return kernel_meta(open(s_path).read())

    with concurrent.futures.ThreadPoolExecutor(max_workers=len(units)) as pool:
        metas = list(pool.map(one, units))
    union = {}
    for unit, m in zip(units, metas):
        assert not set(m) & set(union), (unit, sorted(set(m) & set(union)), "a kernel in two units")
        union.update(m)
    return union


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    m = units_meta(UNITS, tmp_path_factory.mktemp("xyz_codeobj"))
    assert len(m) >= 40, sorted(m)
    return m


def one(meta, key):
    ks = [v for k, v in meta.items() if key in k]
    assert len(ks) == 1, (key, sorted(meta))
    return ks[0]


@pytest.mark.parametrize("io", [1, 2])
def test_forward_kernel_spills_nothing(meta, io):
    k = one(meta, "k_lift_xyz_fwdILi%dEE" % io)
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 128 and k["max_flat_workgroup_size"] >= 1024


@pytest.mark.parametrize("io", [1, 2])
def test_inverse_bench_path_spills_less_than_before(meta, io):
    k = one(meta, "k_lift_xyz_invILi%dELb1ELb0E" % io)
    spills, scratch = k["vgpr_spill_count"], k["private_segment_fixed_size"]
    print("k_lift_xyz_inv<%d, true, false>: %d VGPRs, %d spilled, %d SGPRs spilled, %d bytes of scratch"
          % (io, k["vgpr_count"], spills, k["sgpr_spill_count"], scratch))
    assert k["vgpr_count"] <= 128 and k["max_flat_workgroup_size"] >= 1024
    assert spills < PARENT[io][0] and scratch < PARENT[io][1], (spills, scratch, "not below the figures before the change")
    assert spills <= REACHED[io][0] and scratch <= REACHED[io][1], (spills, scratch, "above what the change reached")


def test_no_other_kernel_gains_scratch(meta):
    seen = set()
    for name, k in meta.items():
        key = next((s for s in SCRATCH_BEFORE if s in name), None)
        seen.add(key)
        assert k["private_segment_fixed_size"] <= (SCRATCH_BEFORE[key] if key else 0), (name, k["private_segment_fixed_size"])
    assert seen >= set(SCRATCH_BEFORE), "a kernel of the table is gone: " + str(set(SCRATCH_BEFORE) - seen)
