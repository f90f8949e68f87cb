"""CPU (hipcc cross-compiles gfx950 here): registers, spills and scratch of k_emit_pixels (sperr_amd/csrc/speck_enc.hip),
read from the code object metadata of the ISA the compiler emits with the Makefile's flags.

The kernel's waits are LDS round trips, a block scan and barriers: what covers them is resident wavefronts, and those are
set by the vector registers a thread takes (LDS, about 6 KB a workgroup, does not limit them).  Before the 32-bit pass
held its samples as plane masks (pix_planes.h) the two instantiations took 94 / 112 VGPRs -- five and four wavefronts per
SIMD.  The 32-bit pass now asks the compiler for seven (at most 72 VGPRs) and gets them without a spill; eight (64) still
spills one 64-bit value inside the plane loop, which is why it is not asked for.  The figures reached are pinned so that
a later change cannot give them back silently.  Metadata only: the instruction text is not searched."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "sperr_amd", "csrc", "speck_enc.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-value", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# mangled template argument -> VGPRs before the change / what the change reached
PARENT = {"Ij": 94, "Im": 112}
REACHED = {"Ij": 72, "Im": 102}


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
    s_path = str(tmp_path_factory.mktemp("emit_codeobj") / "speck_enc.s")
    r = subprocess.run(["hipcc", *FLAGS, "-S", SRC, "-o", s_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    m = kernel_meta(open(s_path).read())
    assert len(m) >= 20, sorted(m)
    return m


@pytest.mark.parametrize("ct", ["Ij", "Im"], ids=["uint32", "uint64"])
def test_emit_pixels_registers(meta, ct):
    ks = [v for k, v in meta.items() if "k_emit_pixels" + ct + "E" in k]
    assert len(ks) == 1, sorted(meta)
    k = ks[0]
    print("k_emit_pixels<%s>: %d VGPRs, %d AGPRs, %d SGPRs, %d bytes of scratch, %d bytes of LDS"
          % ({"Ij": "uint32_t", "Im": "uint64_t"}[ct], k["vgpr_count"], k["agpr_count"], k["sgpr_count"],
             k["private_segment_fixed_size"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0, k
    assert k["vgpr_count"] <= PARENT[ct], (k["vgpr_count"], "above the figure before the change")
    assert k["vgpr_count"] <= REACHED[ct], (k["vgpr_count"], "above what the change reached")


def test_32_bit_pass_has_seven_wavefronts_per_simd(meta):
    k = [v for n, v in meta.items() if "k_emit_pixelsIjE" in n][0]
    # 512 VGPRs per SIMD lane, allocated in blocks of 8
    assert 512 // ((k["vgpr_count"] + 7) // 8 * 8) >= 7, k["vgpr_count"]
    assert k["group_segment_fixed_size"] * 7 <= 160 * 1024, "LDS would limit the seven workgroups of a compute unit"
