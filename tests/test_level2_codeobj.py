"""CPU (hipcc cross-compiles gfx950 here): the kernels of the fused second transform level (k_lift2_fwd in
sperr_amd/csrc/lift_xyz_fwd.hip, k_lift2_inv<SG> in lift_xyz_inv.hip) in the code object metadata of the ISA the
compiler emits with the Makefile's flags.

They wrap the bodies of the finest-level kernels at half the positions per thread (rows of at most 128 samples): one
workgroup of 1024 threads per compute unit leaves a thread 128 VGPRs, and at that size neither direction may spill a
vector register or use a byte of scratch -- a reload inside the slice loop waits for every prefetch and store in flight
(DESIGN.md section 2b), and test_xyz_codeobj.py allows a kernel that is not in its table no scratch at all."""
import shutil

import pytest

from test_xyz_codeobj import LIFT2_UNITS, UNITS, units_meta

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# substring of the mangled name -> what it is
KERNELS = {"k_lift2_fwdE": "k_lift2_fwd", "k_lift2_invILb0EE": "k_lift2_inv<false>", "k_lift2_invILb1EE": "k_lift2_inv<true>"}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    return units_meta(LIFT2_UNITS, tmp_path_factory.mktemp("level2_codeobj"))


@pytest.mark.parametrize("key", list(KERNELS))
def test_level2_kernel_fits_its_registers(meta, key):
    ks = [v for k, v in meta.items() if key in k]
    assert len(ks) == 1, (key, sorted(meta))
    k = ks[0]
    print("%s: %d VGPRs, %d spilled, %d SGPRs (%d spilled), private segment %d bytes"
          % (KERNELS[key], k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_count"], k["sgpr_spill_count"],
             k["private_segment_fixed_size"]))
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 128 and k["max_flat_workgroup_size"] >= 1024, k


def test_no_level2_kernel_answers_to_a_finest_level_name(meta):
    """test_xyz_codeobj.py picks the finest-level kernels by substring of the mangled name"""
    for name in meta:
        if "k_lift2_" in name:
            assert "k_lift_xyz_" not in name, name
    # ... among the kernels of these very units: the ones it compiles include both of this test's
    assert set(LIFT2_UNITS) <= set(UNITS) and LIFT2_UNITS == ["lift_xyz_fwd.hip", "lift_xyz_inv.hip"]
