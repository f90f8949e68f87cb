"""CPU: the five entry points of the interleaved-fields calls are declared in include/sperr_hip.h, listed in
api.EXPORTS with argument types, and exported by the library as built for gfx950; the header, with the new struct,
still compiles as C.  No compute call is made: there is no GPU here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sperrhip_compress_fields_dev", "sperrhip_decompress_fields_dev", "sperrhip_quality_fields_dev",
         "sperrhip_fields_gather_dev", "sperrhip_fields_scatter_dev"]


def test_fields_entry_points_declared_listed_and_exported():
    from sperr_amd import api
    header = open(os.path.join(ROOT, "include", "sperr_hip.h")).read()
    declared = set(re.findall(r"\b(sperr(?:hip)?_[a-z0-9_]+)\s*\(", header))
    assert "typedef struct sperrhip_fields" in header
    if not os.path.exists(api.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sperr_amd", "csrc"), "-j4"])
    raw = ctypes.CDLL(api.LIB_PATH)
    lib = api.load_library()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/sperr_hip.h"
        assert name in api.EXPORTS, f"{name} is not in api.EXPORTS"
        assert hasattr(raw, name), f"{name} is not exported by {api.LIB_PATH}"
        fn = getattr(lib, name)
        assert fn.argtypes and fn.restype is ctypes.c_int, f"{name} has no argument types in api.load_library"
    # the struct of the binding is the header's: three size_t
    assert [f[0] for f in api.Fields._fields_] == ["stride_x", "pitch_y", "pitch_z"]
    assert ctypes.sizeof(api.Fields) == 3 * ctypes.sizeof(ctypes.c_size_t)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not on PATH")
def test_header_still_compiles_as_c():
    src = '#include "sperr_hip.h"\nint main(void){ sperrhip_fields l = {4, 16, 64}; ' \
          'return sperrhip_compress_fields_dev && sperrhip_fields_scatter_dev && l.stride_x == 4 ? 0 : 1; }\n'
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-address", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(), check=True)
