"""CPU (hipcc cross-compiles gfx950 here): registers, LDS and scratch of every instantiation of k_series_fwd and
k_series_inv (series.hip), read from the code object metadata of the ISA the compiler emits with the Makefile's flags
-- the figures DESIGN.md section 0l states.  No instantiation takes a private segment, spills or uses LDS; registers
stay at or below what was measured when they were written.  Metadata only."""
import os
import shutil
import subprocess

import pytest

from test_emit_codeobj import FLAGS, kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# (kernel, element type as mangled, l) -> VGPRs stated in DESIGN.md
STATED = {("fwd", "f"): (22, 42, 70, 138, 138), ("fwd", "d"): (16, 26, 42, 74, 138),
          ("inv", "f"): (26, 42, 66, 106, 178), ("inv", "d"): (18, 26, 38, 58, 94)}
CASES = [(k, t, l) for (k, t) in sorted(STATED) for l in range(5)]


@pytest.fixture(scope="module")
def metas(tmp_path_factory):
    s_path = str(tmp_path_factory.mktemp("series_codeobj") / "series.s")
    r = subprocess.run(["hipcc", *FLAGS, "-S", os.path.join(ROOT, "sperr_amd", "csrc", "series.hip"), "-o", s_path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return kernel_meta(open(s_path).read())


def test_every_instantiation_is_there(metas):
    assert len([k for k in metas if "k_series_" in k]) == len(CASES), sorted(metas)


@pytest.mark.parametrize("kern,elem,l", CASES)
def test_no_scratch_no_lds_and_the_stated_registers(metas, kern, elem, l):
    name = "12k_series_%sI%sLi%dEE" % (kern, elem, l)
    ks = [v for k, v in metas.items() if name in k]
    assert len(ks) == 1, sorted(metas)
    k = ks[0]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of scratch, %d bytes of LDS"
          % (name, k["vgpr_count"], k["sgpr_count"], k["private_segment_fixed_size"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["agpr_count"] == 0, k
    assert k["vgpr_count"] <= STATED[(kern, elem)][l], k
