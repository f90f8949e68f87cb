"""CPU (hipcc cross-compiles gfx950 here): registers, LDS and scratch of k_lis_bits and k_plane_table
(sperr_amd/csrc/speck_enc.hip), read from the code object metadata of the ISA the compiler emits with the Makefile's flags
-- the figures DESIGN.md sections 0j and 3 state.  The kernel takes no private segment (the issue's condition), and its
registers stay at or below what was measured when it was written.  Metadata only: the instruction text is not searched."""
import shutil

import pytest

from test_emit_codeobj import meta   # noqa: F401  (the fixture: one compile of speck_enc.hip to ISA)

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# (VGPRs, bytes of LDS) stated in DESIGN.md
STATED = {"k_lis_bits": (27, 768), "k_plane_table": (26, 0)}


@pytest.mark.parametrize("name", sorted(STATED))
def test_no_scratch_and_the_stated_registers(meta, name):   # noqa: F811
    ks = [v for k, v in meta.items() if name in k]
    assert len(ks) == 1, sorted(meta)
    k = ks[0]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of scratch, %d bytes of LDS"
          % (name, k["vgpr_count"], k["sgpr_count"], k["private_segment_fixed_size"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["agpr_count"] == 0, k
    assert k["vgpr_count"] <= STATED[name][0] and k["group_segment_fixed_size"] == STATED[name][1], k
