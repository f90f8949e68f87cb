"""The drop-in, literally: include/compat/ carries the reference's header names (SPERR_C_API.h with
the declarations inside namespace C_API for C++, SPERR3D_OMP_C.h, SPERR3D_OMP_D.h, SPECK3D_FLT.h,
SPECK2D_FLT.h, SPERR3D_Stream_Tools.h, sperr_helper.h, SperrConfig.h), sperr_amd/libSPERR.so is the
reference's link name (the reference's SPERR.pc.in: -lSPERR).

CPU: the reference's own examples/C_API/2d.c and 3d.c, compiled IN PLACE and unmodified with
-Iinclude/compat -lSPERR by `make -C oracle examples` (part of build() where the reference's sources are
present; the binaries stay in oracle/_ref/examples), link against libSPERR.so; a C++ caller spelling C_API::sperr_comp_3d and using the
driver classes + host helpers under their reference names compiles, links, and its helpers agree
with the oracle / reference.  GPU: the example binaries (built by `make -C oracle examples`, they
travel in oracle/_ref/) and the C++ caller run on the device and produce the oracle's bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sperr_amd.synth import turbulence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "oracle", "_ref", "examples")
COMPAT = os.path.join(ROOT, "include", "compat")
LIBDIR = os.path.join(ROOT, "sperr_amd")
LINK = ["-L" + LIBDIR, "-lSPERR", "-L/opt/rocm/lib", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]


def ensure_alias():
    alias = os.path.join(LIBDIR, "libSPERR.so")
    if not os.path.exists(alias):
        os.symlink("libsperr_hip.so", alias)


def build_caller(tmp_path):
    ensure_alias()
    exe = tmp_path / "compat_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + COMPAT,
                           os.path.join(ROOT, "tests", "cpp", "compat_check.cpp"), "-o", str(exe), *LINK])
    return exe


@pytest.mark.parametrize("src", ["2d.c", "3d.c"])
def test_reference_examples_compile_in_place_unmodified(src):
    # built by oracle/Makefile `examples` with the build line of the reference's examples/C_API/Makefile, the two
    # directories replaced (make fails the build where they do not compile)
    exe = os.path.join(EXAMPLES, src[:-2] + ".out")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/examples not built (build() builds them where the reference's sources are present)")
    ensure_alias()
    needed = subprocess.check_output(["readelf", "-d", str(exe)], text=True)
    assert "libSPERR.so" in needed
    undefined = subprocess.check_output(["nm", "-u", str(exe)], text=True)
    want = ["sperr_comp_2d", "sperr_decomp_2d"] if src == "2d.c" else ["sperr_comp_3d", "sperr_decomp_3d"]
    for sym in want + ["sperr_parse_header"]:
        assert sym in undefined


def test_pkgconfig_file_names_the_alias():
    pc = os.path.join(LIBDIR, "pkgconfig", "SPERR.pc")
    if not os.path.exists(pc):
        pytest.skip("not built (make -C sperr_amd/csrc)")
    text = open(pc).read()
    assert "-lSPERR" in text and "include/compat" in text and "Name: SPERR" in text


def test_cpp_caller_with_reference_names_builds_and_helpers_agree(tmp_path, oracle):
    exe = build_caller(tmp_path)
    out = subprocess.run([str(exe), "helpers"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "version 0.8.5"      # the reference's CMakeLists.txt:5
    # geometry against the oracle's restatement (pinned to the reference, tests/test_oracle_vs_ref.py)
    chunks = [tuple(map(int, l.split()[1:])) for l in lines if l.startswith("chunk ")]
    want = oracle.chunk_volume((1000, 300, 70), (256, 256, 256))
    assert chunks == [tuple(int(v) for v in c) for c in want]
    xf = {int(l.split()[1]): (int(l.split()[2]), int(l.split()[4])) for l in lines if l.startswith("xforms ")}
    assert xf[8] == (0, 3) and xf[9] == (1, 4) and xf[256] == (5, 8) and xf[4096] == (6, 12) and xf[250] == (5, 8)
    dy = {tuple(map(int, l.split()[1:4])): int(l.split()[4]) for l in lines if l.startswith("dyadic ")}
    assert dy[(256, 256, 256)] == 5 and dy[(128, 128, 41)] == -1 and dy[(17, 17, 17)] == 2 and dy[(999, 999, 1)] == -1
    res = [tuple(map(int, l.split()[1:])) for l in lines if l.startswith("res ")]
    assert res[:5] == [(8,) * 3, (16,) * 3, (32,) * 3, (64,) * 3, (128,) * 3]
    assert (500, 500, 1) in res and (16, 16, 1) in res and (9, 9, 9) in res
    volres = [tuple(map(int, l.split()[1:])) for l in lines if l.startswith("volres ")]
    assert volres == [(32, 16, 8), (64, 32, 16), (128, 64, 32), (256, 128, 64)]
    assert "volres_indivisible 0" in lines
    assert "bools 10100100 147" in lines and "same_psnr_inf 1" in lines
    # statistics: the same blocked float sums in numpy
    i = np.arange(20000, dtype=np.uint64)
    a = (((i * 2654435761) % (1 << 32)) % 1000).astype(np.float32) / np.float32(7.0)
    c = a + (((i * 40503) % (1 << 32)) % 13).astype(np.float32) * np.float32(1e-3)
    d = np.abs(a - c)
    sq = d * d

    def blocked(v, block):
        total = np.float32(0)
        n = len(v) // block
        for b in range(n):
            s = np.float32(0)
            for x in v[b * block:(b + 1) * block]:
                s = np.float32(s + x)
            total = np.float32(total + s)
        s = np.float32(0)
        for x in v[n * block:]:
            s = np.float32(s + x)
        return np.float32(total + s)

    mse = np.float32(blocked(sq, 8192) / np.float32(len(a)))
    st = [float(x) for x in next(l for l in lines if l.startswith("stats ")).split()[1:]]
    assert st[0] == pytest.approx(float(np.sqrt(mse)), rel=1e-6)
    assert st[1] == pytest.approx(float(d.max()), rel=1e-7)
    rng = np.float32(a.max() - a.min())
    assert st[2] == pytest.approx(float(np.float32(10) * np.log10(rng * rng / mse)), rel=1e-6)
    assert st[3] == float(a.min()) and st[4] == pytest.approx(float(a.max()), rel=1e-7)


@pytest.mark.gpu
def test_reference_examples_run_on_the_device(tmp_path, oracle):
    """examples/C_API/3d.c and 2d.c as the reference ships them (binaries from `make -C oracle
    examples`), on the GPU through libSPERR.so: output.stream and output.data are the oracle's."""
    ex = os.path.join(ROOT, "oracle", "_ref", "examples")
    if not os.path.exists(os.path.join(ex, "3d.out")):
        pytest.skip("oracle/_ref/examples not built (needs the reference tree, dev container)")
    ensure_alias()
    vol = turbulence((96, 64, 80)).astype(np.float64)          # z y x; 3d.c asks for 256^3 chunks: one chunk
    vol.tofile(tmp_path / "vol.f64")
    for mode, q in ((1, 2.6), (2, 102.5), (3, 4e-5)):        # the cases of examples/C_API/test.sh
        p = subprocess.run([os.path.join(ex, "3d.out"), str(tmp_path / "vol.f64"), "80", "64", "96", str(mode),
                            repr(q), "-d"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        want = oracle.comp_3d(vol, (256, 256, 256), mode, q)
        assert (tmp_path / "output.stream").read_bytes() == want
        back = np.fromfile(tmp_path / "output.data", dtype=np.float64)
        assert np.array_equal(back.view(np.uint64), oracle.decomp_3d(want, False).ravel().view(np.uint64))
    img = np.ascontiguousarray(turbulence((4, 150, 201))[1])    # y x, float
    img.tofile(tmp_path / "img.f32")
    for mode, q in ((1, 2.5), (2, 90.0), (3, 1e-3)):
        p = subprocess.run([os.path.join(ex, "2d.out"), str(tmp_path / "img.f32"), "201", "150", str(mode), repr(q)],
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        want = oracle.comp_2d(img, mode, q, True)
        assert (tmp_path / "output.stream").read_bytes() == want
        back = np.fromfile(tmp_path / "output.data", dtype=np.float32)
        assert np.array_equal(back.view(np.uint32), oracle.decomp_2d(want[10:], img.shape, True).ravel().view(np.uint32))


@pytest.mark.gpu
def test_cpp_caller_with_reference_names_runs_on_the_device(tmp_path, oracle):
    exe = build_caller(tmp_path)
    dims, chunks = (64, 48, 40), (32, 32, 32)     # x y z
    v = turbulence(dims[::-1])
    v.tofile(tmp_path / "vol.f32")
    p = subprocess.run([str(exe), "run", str(tmp_path / "vol.f32"), *map(str, dims), *map(str, chunks), str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    pwe = oracle.comp_3d(v, chunks, 3, 1e-3)
    assert (tmp_path / "capi_pwe").read_bytes() == pwe
    back = np.fromfile(tmp_path / "capi_pwe_f32", dtype=np.float32)
    assert np.array_equal(back.view(np.uint32), oracle.decomp_3d(pwe, True).ravel().view(np.uint32))
    linf = float(next(l for l in p.stdout.splitlines() if l.startswith("linfty ")).split()[1])
    assert linf <= 1e-3 * (1 + 1e-6)
    assert (tmp_path / "capi_trunc50").read_bytes() == oracle.trunc_3d(pwe, 50)
    rate = oracle.comp_3d(v, chunks, 1, 2.0)
    assert (tmp_path / "omp_c_bpp2").read_bytes() == rate
    vol = np.fromfile(tmp_path / "omp_d_f64", dtype=np.float64)
    assert np.array_equal(vol.view(np.uint64), oracle.decomp_3d(rate, False).ravel().view(np.uint64))
    img = np.ascontiguousarray(v[0])
    assert (tmp_path / "speck2d_psnr90").read_bytes() == oracle.comp_2d(img, 2, 90.0, False)
