"""CPU (hipcc cross-compiles gfx950 here): registers, spills, scratch and static LDS of the decoder's list kernels
(k_lis_l0, k_lis_l1, k_lis_l2, k_lis_hi: sperr_amd/csrc/speck_dec.hip; k_lis_mx: speck_mx.hip), read from the code object
metadata of the ISA the compiler emits with the Makefile's flags.  Only the metadata block is read.

The three block-parallel kernels are built from shared phases (lis_chain.h, lis_token.h).  Their occupancy is set by
attribute -- two workgroups of 1024 threads a compute unit for k_lis_l0: 64 VGPRs a thread, not one more; two of 512
for the others: 128 -- and k_lis_l0 sat at exactly 64 with two of them spilled before the phases were shared.  The
ceilings below are the figures of the kernels as they were written out one by one (measured at the commit before the
skeleton, with the same flags), so that a change to a shared phase cannot cost one of the kernels registers, scratch or
LDS silently.  The two region kernels (k_lis_hi, k_lis_mx) share their protocol half the same way (lis_region.h);
k_lis_mx's ceilings are its figures at the commit before that header, plain and with stamps."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")
SRCS = {"speck_dec.hip": 25, "speck_mx.hip": 2}   # file: kernels it holds at least
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-value", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# kernel: (VGPRs the occupancy attribute allows, spilled VGPRs, bytes of scratch, bytes of static LDS) before the skeleton
# (SGPRs spilled then: 20, 0, 4, 89 -- they go to VGPR lanes, which the other figures bound)
CEILING = {
    "k_lis_l0E": (64, 2, 12, 6400),
    "k_lis_l1E": (128, 0, 0, 6496),
    "k_lis_l2E": (128, 0, 0, 10256),
    "k_lis_hiIjE": (128, 0, 16, 11376),
    "k_lis_hiImE": (128, 0, 16, 11376),
    "k_lis_mxILb0E": (126, 0, 0, 20912),
    "k_lis_mxILb1E": (128, 19, 84, 20928),
}


def kernel_meta(s_text):
    """{kernel symbol: {key: int}} from the code object metadata at the end of the ISA file"""
    meta = {}
    for m in re.finditer(r"^\s+- \.agpr_count:.*?(?=^\s+- \.agpr_count:|\Z)", s_text, flags=re.S | re.M):
        blk = m.group(0)
        nm = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[nm] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    return meta


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lis_codeobj")
    procs = {src: subprocess.Popen(["hipcc", *FLAGS, "-S", os.path.join(CSRC, src), "-o", str(tmp / (src + ".s"))],
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for src in SRCS}
    m = {}
    for src, proc in procs.items():
        out = proc.communicate()[0]
        assert proc.returncode == 0, out[-3000:]
        one_file = kernel_meta(open(tmp / (src + ".s")).read())
        assert len(one_file) >= SRCS[src], sorted(one_file)
        m.update(one_file)
    return m


def one(meta, key):
    ks = [v for k, v in meta.items() if key in k]
    assert len(ks) == 1, (key, sorted(meta))
    return ks[0]


@pytest.mark.parametrize("key", sorted(CEILING))
def test_list_kernel_stays_within_its_figures(meta, key):
    k = one(meta, key)
    vgprs, spills, scratch, lds = CEILING[key]
    print("%s: %d VGPRs, %d spilled, %d SGPRs spilled, %d bytes of scratch, %d bytes of static LDS"
          % (key, k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"],
             k["group_segment_fixed_size"]))
    assert k["vgpr_count"] <= vgprs, k
    assert k["vgpr_spill_count"] <= spills, k
    assert k["private_segment_fixed_size"] <= scratch, k
    assert k["group_segment_fixed_size"] <= lds, k


def test_no_other_kernel_gains_scratch(meta):
    seen = set()
    for name, k in meta.items():
        key = next((s for s in CEILING if s in name), None)
        seen.add(key)
        assert k["private_segment_fixed_size"] <= (CEILING[key][2] if key else 0), (name, k["private_segment_fixed_size"])
    assert seen >= set(CEILING), "a kernel of the table is gone: " + str(set(CEILING) - seen)
