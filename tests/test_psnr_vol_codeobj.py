"""CPU (hipcc cross-compiles gfx950 here): registers, LDS and scratch of k_mse_ladder, k_mse_ladder_pick (xform.hip) and
k_vol_range (psnr_vol.hip), read from the code object metadata of the ISA the compiler emits with the Makefile's flags
-- the figures DESIGN.md section 0k states.  No kernel takes a private segment or spills; the ladder keeps k_mse_strides'
LDS tile; registers stay at or below what was measured when they were written.  Metadata only."""
import os
import shutil
import subprocess

import pytest

from test_emit_codeobj import FLAGS, kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# kernel symbol fragment -> (unit, VGPRs, bytes of LDS) stated in DESIGN.md
STATED = {"12k_mse_ladderE": ("xform.hip", 84, 33280), "17k_mse_ladder_pickE": ("xform.hip", 18, 0),
          "11k_vol_rangeIfLb1EE": ("psnr_vol.hip", 51, 80), "11k_vol_rangeIdLb1EE": ("psnr_vol.hip", 42, 80),
          "11k_vol_rangeIfLb0EE": ("psnr_vol.hip", 22, 80), "11k_vol_rangeIdLb0EE": ("psnr_vol.hip", 26, 80)}


@pytest.fixture(scope="module")
def metas(tmp_path_factory):
    d = tmp_path_factory.mktemp("psnr_vol_codeobj")
    out = {}
    for unit in ("xform.hip", "psnr_vol.hip"):
        s_path = str(d / (unit + ".s"))
        r = subprocess.run(["hipcc", *FLAGS, "-S", os.path.join(ROOT, "sperr_amd", "csrc", unit), "-o", s_path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        out[unit] = kernel_meta(open(s_path).read())
    return out


@pytest.mark.parametrize("name", sorted(STATED))
def test_no_scratch_and_the_stated_registers(metas, name):
    unit, vgprs, lds = STATED[name]
    ks = [v for k, v in metas[unit].items() if name in k]
    assert len(ks) == 1, sorted(metas[unit])
    k = ks[0]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of scratch, %d bytes of LDS"
          % (name, k["vgpr_count"], k["sgpr_count"], k["private_segment_fixed_size"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["agpr_count"] == 0, k
    assert k["vgpr_count"] <= vgprs and k["group_segment_fixed_size"] == lds, k
