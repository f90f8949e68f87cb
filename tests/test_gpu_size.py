"""GPU (-m gpu): compression to a byte target (budget.h) -- the plane table, the survey, the dealt
container.  The yardsticks are the CPU oracle and tests/size_model.py; every compare is on integers, bytes or bit patterns.

  table      sperrhip_speck3d_plane_bits_dev: end[p] equals the total_bits field of oracle.speck3d_encode(coef >> p, sign)
             at full depth for every p -- shifting the magnitudes right by p leaves exactly the decisions and bits of the
             planes >= p.  16^3 (an octree), 17^3 and 20 x 18 x 16 (any-shape sets); the quantised goldens and the
             tree-aligned patterns of tests/coef_cases.py
  survey     a ragged volume of two chunk shapes: every chunk's row is the stage call's on the chunk's own coefficients,
             q and the plane count are those of the fixed-rate container's chunk headers
  container  a 64^3 volume in 32^3 chunks whose chunks differ a thousandfold in amplitude, fp32 and fp64, at 0.5, 1 and
             2 bits per sample of the volume: the budgets are the model's on the surveyed table; chunk stream c is
             oracle.chunk_compress_rate(chunk_c, (b_c + 0.5) / N_c) byte for byte; the length is within #chunks + 1
             bytes below the target; the oracle (and the reference, where it is built) opens it; decompress,
             decompress_box and decompress(pct=50) are the oracle's bits
  quality    the dealt container's mean squared error is strictly below that of the fixed-rate container at the
             smallest rate whose container is at least as long
  threshold  q_c 2^p of the last plane every chunk completes lies within a factor of 2 across the chunks that are
             neither at the 8-bit floor nor coded in full
  edges      a constant chunk; an all-constant volume; a target too small (refused, the destination untouched); a target
             beyond full depth (a shorter container, every chunk in full, no 64-bit pass); a homogeneous volume
  children   the 1-bpp case with SPERR_HIP_ARENA_MAX_MB set (survey and encode in one batch per chunk) and with
             SPERR_HIP_POISON=0xFF, each in a process of its own"""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import coef_cases as cc
import size_model as sm
from sperr_amd.farm import chunk_grid, split_container

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_U = np.uint64
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    return SperrHip()


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    return bytes(t.cpu().numpy())


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- a. the plane table against the oracle -------------------------------------------------------------------------------

SHAPES = {"16": (16, 16, 16), "17": (17, 17, 17), "20x18x16": (16, 18, 20)}   # (z, y, x)
# (every 32-bit case of the table; the two wide_* cases need the 64-bit pass, which the call refuses)
PATTERNS = ("tiers2_all", "tiers4_one", "tiers8_all", "checker2", "checker8", "stagger8_one", "front4", "all_one",
            "dense_top32", "last_only", "first_only")


def quantised(oracle, vol):
    """the coefficients and sign words of a chunk, quantised with the fixed-rate step"""
    v, _, const = oracle.condition(vol.astype(np.float64))
    assert not const
    w = oracle.dwt3d(v)
    q = float(np.abs(w).max()) / float(2 ** 32 - 1)
    coef, sign, width = oracle.quantize(w, q)
    assert int(coef.max()) < 2 ** 32
    return coef, sign


def table_case(oracle, data, shape):
    if data == "vort_crop":
        vol = np.fromfile(os.path.join(GOLD, "vort_crop.f32"), dtype=np.float32).reshape(33, 36, 40)
        return quantised(oracle, vol[3:3 + shape[0], 5:5 + shape[1], 7:7 + shape[2]])
    if data == "wmag17":
        return quantised(oracle, np.fromfile(os.path.join(GOLD, "wmag17.f32"), dtype=np.float32).reshape(17, 17, 17))
    coef, sign, wide = cc.case(data, shape)
    assert not wide
    return coef, sign


def oracle_table(oracle, coef, sign):
    """(end[p] for p < 64, nbp): full-depth bit counts of the magnitudes shifted right by p"""
    end = np.zeros(64, dtype=np.uint64)
    nbp = 0
    for p in range(64):
        c = np.ascontiguousarray(coef >> _U(p))
        if not c.any():
            break
        s = oracle.speck3d_encode(c, sign, 0)
        end[p] = struct.unpack_from("<Q", s, 1)[0]
        if p == 0:
            nbp = s[0]
    return end, nbp


TABLE_CASES = ([(d, k) for k in SHAPES for d in ("vort_crop",) + PATTERNS] + [("wmag17", "17")])


@pytest.mark.parametrize("data,shape", TABLE_CASES, ids=["%s-%s" % c for c in TABLE_CASES])
def test_plane_table_is_the_oracles_bit_count_of_every_plane(eng, oracle, data, shape):
    coef, sign = table_case(oracle, data, SHAPES[shape])
    want, nbp = oracle_table(oracle, coef, sign)
    got, got_nbp = eng.speck3d_plane_bits(cuda(coef.astype(np.uint32).view(np.int32)), cuda(sign.view(np.int64)))
    print(data, shape, "planes", nbp, "bits of the whole stream", int(want[0]))
    assert got_nbp == nbp
    assert np.array_equal(got, want), [(p, int(g), int(w)) for p, (g, w) in enumerate(zip(got, want)) if g != w]


def test_plane_table_refuses_wide_coefficients_and_slices(eng):
    import ctypes as C
    coef, sign, _ = cc.case("all_one", (16, 16, 16))
    d, s = cuda(coef.view(np.int64)), cuda(sign.view(np.int64))
    end, nbp = np.zeros(64, dtype=np.uint64), C.c_int(0)
    st = eng._stream()
    assert eng.lib.sperrhip_speck3d_plane_bits_dev(d.data_ptr(), 8, s.data_ptr(), 16, 16, 16, end.ctypes.data, C.byref(nbp), st) == -1
    assert eng.lib.sperrhip_speck3d_plane_bits_dev(d.data_ptr(), 4, s.data_ptr(), 16, 16, 0, end.ctypes.data, C.byref(nbp), st) == -1


# ---- b. the survey -----------------------------------------------------------------------------------------------------

def chunk_of(vol, box):
    x0, lx, y0, ly, z0, lz = box
    return np.ascontiguousarray(vol[z0:z0 + lz, y0:y0 + ly, x0:x0 + lx])


def test_survey_of_a_ragged_volume(eng, oracle):
    vol = np.fromfile(os.path.join(GOLD, "vort_crop.f32"), dtype=np.float32).reshape(33, 36, 40)
    chunks = (20, 18, 16)
    boxes = chunk_grid(vol.shape, chunks)
    assert len({(b[1], b[3], b[5]) for b in boxes}) == 2
    sv = eng.size_survey(cuda(vol), chunks)
    _, _, _, parts = split_container(host(eng.compress(cuda(vol), chunks, 4.0)))
    assert len(parts) == len(boxes) == len(sv["q"])
    for c, (box, part) in enumerate(zip(boxes, parts)):
        assert part[0] == 0x80 and not sv["is_const"][c]
        q = struct.unpack_from("<d", part, 9)[0]
        assert sv["q"][c] == q and sv["nbp"][c] == part[17], c
        ck = chunk_of(vol, box).astype(np.float64)
        v, _, _ = oracle.condition(ck)
        coef, sign, _ = oracle.quantize(oracle.dwt3d(v), q)
        end, nbp = eng.speck3d_plane_bits(cuda(coef.astype(np.uint32).view(np.int32)), cuda(sign.view(np.int64)))
        assert nbp == sv["nbp"][c] and np.array_equal(end[:32], sv["end"][c]) and not end[32:].any(), c


# ---- c. the container --------------------------------------------------------------------------------------------------

CHUNKS = (32, 32, 32)
AMP = {(0, 0, 0): 1.0, (1, 1, 0): 0.1}


def plume(dtype, const_chunk=False):
    """64^3: sin(x / 5) cos(y / 7) sin(z / 6 + 0.3) plus 5 % white noise; the 32^3 chunk at the origin as it is, one
    scaled by 0.1, six by 1e-3 (const_chunk: the last one a constant)"""
    def make():
        rng = np.random.default_rng(7)
        z, y, x = np.meshgrid(*(np.arange(64),) * 3, indexing="ij")
        v = np.sin(x / 5.0) * np.cos(y / 7.0) * np.sin(z / 6.0 + 0.3) + 0.05 * rng.standard_normal((64,) * 3)
        for k in range(2):
            for j in range(2):
                for i in range(2):
                    v[k * 32:(k + 1) * 32, j * 32:(j + 1) * 32, i * 32:(i + 1) * 32] *= AMP.get((k, j, i), 1e-3)
        if const_chunk:
            v[32:, 32:, 32:] = 0.25
        v = np.ascontiguousarray(v.astype(dtype))
        v.setflags(write=False)
        return v
    return cached(("plume", np.dtype(dtype).name, const_chunk), make)


def table_of(sv):
    return sv["q"], sv["nbp"].astype(np.int64), sv["end"], sv["is_const"]


def dealt(eng, vol, target):
    """(container bytes, budgets, survey) of a volume at a byte target"""
    def make():
        d = cuda(vol)
        sv = eng.size_survey(d, CHUNKS)
        c, b = eng.compress_to_size(d, CHUNKS, target, return_plan=True)
        return host(c), [int(v) for v in b], sv
    return cached(("dealt", id(vol), target), make)


def check_container(eng, oracle, vol, target, container, budgets, sv):
    n = len(budgets)
    nconst = int(np.count_nonzero(sv["is_const"]))
    W = sm.payload_bits(target, n, nconst)
    want, star, nxt = sm.deal(table_of(sv), W)
    print("target", target, "W", W, "T*", star, "T'", nxt, "budgets", budgets, "bytes", len(container))
    assert budgets == want
    flags, _, _, parts = split_container(container)
    assert len(parts) == n
    for c, box in enumerate(chunk_grid(vol.shape, CHUNKS)):
        ck = chunk_of(vol, box).astype(np.float64)
        if sv["is_const"][c]:
            assert len(parts[c]) == 17 and parts[c][0] == 0x81
            continue
        assert bytes(parts[c]) == oracle.chunk_compress_rate(ck, (budgets[c] + 0.5) / ck.size), c
    assert len(container) <= target
    return want


@pytest.mark.parametrize("bpp", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_dealt_container(eng, oracle, dtype, bpp):
    vol = plume(dtype)
    target = int(bpp * vol.size / 8)
    container, budgets, sv = dealt(eng, vol, target)
    check_container(eng, oracle, vol, target, container, budgets, sv)
    assert target - len(container) <= len(budgets) + 1, (target, len(container))
    as_float = dtype == np.float32
    ref_vol = oracle.decomp_3d(container, as_float)
    from oracle import pyoracle
    if pyoracle.have_ref():   # (the reference itself, where it is built)
        ref = cached("ref", pyoracle.Ref)
        assert np.array_equal(bits(ref.decomp_3d(container, as_float)), bits(ref_vol))
    dev = cuda(np.frombuffer(container, dtype=np.uint8))
    got = eng.decompress(dev, output_float=as_float).cpu().numpy()
    assert np.array_equal(bits(got), bits(ref_vol))
    lo, dims = (5, 20, 30), (40, 30, 9)   # (x, y, z): a box that meets all eight chunks
    box = eng.decompress_box(dev, lo, dims, output_float=as_float).cpu().numpy()
    assert np.array_equal(bits(box), bits(np.ascontiguousarray(ref_vol[30:39, 20:50, 5:45])))
    half = eng.decompress(dev, output_float=as_float, pct=50).cpu().numpy()
    assert np.array_equal(bits(half), bits(oracle.decomp_3d(oracle.trunc_3d(container, 50), as_float)))


@pytest.mark.parametrize("bpp", [0.5, 1.0, 2.0])
def test_dealt_container_beats_the_uniform_deal(eng, oracle, bpp):
    """Strictly below the fixed-rate container's error at the smallest rate whose container is at least as long.  A
    fixed-rate container of this volume has 52 + 8 * 26 bytes of headers and 8 * ceil(rate * 32^3 / 8) of payload: the
    rate starts where that reaches the dealt container's length, and is walked up a byte a chunk should it fall short."""
    vol = plume(np.float32)
    target = int(bpp * vol.size / 8)
    container, _, _ = dealt(eng, vol, target)
    d = cuda(vol)
    per = max(1, -(-(len(container) - 52 - 8 * 26) // 8))   # payload bytes a chunk
    rate = per * 8 / 32768.0
    uniform = host(eng.compress(d, CHUNKS, rate))
    while len(uniform) < len(container):
        per += 1
        rate = per * 8 / 32768.0
        uniform = host(eng.compress(d, CHUNKS, rate))
    v64 = vol.astype(np.float64)
    mse_d = float(((oracle.decomp_3d(container, False) - v64) ** 2).mean())
    mse_u = float(((oracle.decomp_3d(uniform, False) - v64) ** 2).mean())
    rng = float(v64.max() - v64.min())
    print("target %d bytes: dealt %d bytes, PSNR %.2f dB; uniform at %.4f bpp %d bytes, PSNR %.2f dB; gain %.2f dB"
          % (target, len(container), 10 * np.log10(rng * rng / mse_d), rate, len(uniform), 10 * np.log10(rng * rng / mse_u),
             10 * np.log10(mse_u / mse_d)))
    assert len(uniform) >= len(container)
    assert mse_d < mse_u


@pytest.mark.parametrize("bpp", [0.5, 1.0, 2.0])
def test_chunks_stop_at_a_common_threshold(eng, bpp):
    vol = plume(np.float32)
    target = int(bpp * vol.size / 8)
    _, budgets, sv = dealt(eng, vol, target)
    thr = [t for t, full in sm.last_plane_threshold(table_of(sv), budgets) if t is not None and not full]
    print("last completed planes' thresholds", thr)
    assert len(thr) >= 2
    assert max(thr) <= 2.0 * min(thr), thr


def test_survey_rows_of_the_32_cube_chunks_are_the_stage_calls(eng, oracle):
    """The container tests' volume: its rows, too, are the stage call's on each chunk's own coefficients -- and so the
    oracle's, by the table test."""
    vol = plume(np.float32)
    sv = eng.size_survey(cuda(vol), CHUNKS)
    assert eng._chunk_count(vol.shape, CHUNKS) == 8 == len(sv["q"])
    for c, box in enumerate(chunk_grid(vol.shape, CHUNKS)):
        v, _, _ = oracle.condition(chunk_of(vol, box).astype(np.float64))
        coef, sign, _ = oracle.quantize(oracle.dwt3d(v), float(sv["q"][c]))
        end, nbp = eng.speck3d_plane_bits(cuda(coef.astype(np.uint32).view(np.int32)), cuda(sign.view(np.int64)))
        assert nbp == sv["nbp"][c] and np.array_equal(end[:32], sv["end"][c]) and not end[32:].any(), c
    want, _ = oracle_table(oracle, coef, sign)   # (the last chunk once more against the oracle itself)
    assert np.array_equal(want[:32], sv["end"][7])


def test_chunks_that_take_the_fused_head(eng, oracle):
    """64^3 chunks take k_head_fused (quantiser, the leaf parents' level of the pyramid and the census in one kernel, which
    also initialises the chunks' states): the survey's rows are the stage call's, which takes the three-kernel head, and
    the dealt container's chunk streams are the oracle's at their budgets -- the budgets reached the fused head."""
    import torch
    one = plume(np.float32)
    vol = np.ascontiguousarray(np.concatenate([one, (one[::-1] * np.float32(0.01))], axis=0))   # (128, 64, 64)
    chunks = (64, 64, 64)
    d = cuda(vol)
    eng.profile(True)
    try:
        sv = eng.size_survey(d, chunks)
        target = vol.size // 8
        c, b = eng.compress_to_size(d, chunks, target, return_plan=True)
        torch.cuda.synchronize()
        names = {k for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)
    assert any("k_head_fused" in k for k in names), sorted(names)
    container, budgets = host(c), [int(v) for v in b]
    want, _, _ = sm.deal(table_of(sv), sm.payload_bits(target, 2, 0))
    print("budgets", budgets)
    assert budgets == want and len(container) <= target and target - len(container) <= 3
    _, _, _, parts = split_container(container)
    for k, box in enumerate(chunk_grid(vol.shape, chunks)):
        ck = chunk_of(vol, box).astype(np.float64)
        v, _, _ = oracle.condition(ck)
        coef, sign, _ = oracle.quantize(oracle.dwt3d(v), float(sv["q"][k]))
        end, nbp = eng.speck3d_plane_bits(cuda(coef.astype(np.uint32).view(np.int32)), cuda(sign.view(np.int64)))
        assert nbp == sv["nbp"][k] and np.array_equal(end[:32], sv["end"][k]) and not end[32:].any(), k
        assert bytes(parts[k]) == oracle.chunk_compress_rate(ck, (budgets[k] + 0.5) / ck.size), k


def test_arrays_too_short_are_refused(eng):
    import ctypes as C
    vol = cuda(plume(np.float32))
    q, nbp, end, ic = np.zeros(8), np.zeros(8, dtype=np.int32), np.zeros((8, 32), dtype=np.uint64), np.full(8, 7, dtype=np.uint8)
    rtn = eng.lib.sperrhip_size_survey_dev(vol.data_ptr(), 1, 64, 64, 64, 32, 32, 32, 7, q.ctypes.data, nbp.ctypes.data,
                                           end.ctypes.data, ic.ctypes.data, eng._stream())
    assert rtn == -1 and (ic == 7).all()
    assert eng.lib.sperrhip_chunk_count(40, 36, 33, 20, 18, 16) == 8 and eng.lib.sperrhip_chunk_count(40, 36, 0, 20, 18, 16) == 0


# ---- d. edges ---------------------------------------------------------------------------------------------------------

def test_a_constant_chunk_inside_the_volume(eng, oracle):
    vol = plume(np.float32, const_chunk=True)
    target = vol.size // 8
    container, budgets, sv = dealt(eng, vol, target)
    assert list(sv["is_const"]) == [False] * 7 + [True] and budgets[7] == 0
    check_container(eng, oracle, vol, target, container, budgets, sv)
    assert target - len(container) <= len(budgets) + 1
    got = eng.decompress(cuda(np.frombuffer(container, dtype=np.uint8))).cpu().numpy()
    assert np.array_equal(bits(got), bits(oracle.decomp_3d(container, True)))


def test_an_all_constant_volume(eng, oracle):
    vol = np.full((64, 64, 64), 3.5, dtype=np.float32)
    c, b = eng.compress_to_size(cuda(vol), CHUNKS, 1000, return_plan=True)
    assert host(c) == oracle.comp_3d(vol, CHUNKS, 1, 2.0) and not b.any()
    with pytest.raises(Exception):
        eng.compress_to_size(cuda(vol), CHUNKS, 20 + 32 + 8 * 17 - 1)


def test_a_target_too_small_is_refused_and_nothing_is_written(eng):
    import torch
    from sperr_amd.api import SperrHipError
    vol = plume(np.float32)
    floor = 20 + 32 + 8 * 26 + 8   # the headers and a payload byte per chunk
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    for target in (floor - 1, 30, 0):
        with pytest.raises(SperrHipError):
            eng.compress_to_size(cuda(vol), CHUNKS, target, out=out)
        assert bool((out == 0xA5).all()), target
    c, b = eng.compress_to_size(cuda(vol), CHUNKS, floor, out=out, return_plan=True)
    assert c.numel() == floor and list(b) == [8] * 8


def test_a_target_beyond_full_depth(eng, oracle):
    vol = plume(np.float32)
    d = cuda(vol)
    sv = eng.size_survey(d, CHUNKS)
    full = [max(8, (int(e) // 8) * 8) for e in sv["end"][:, 0]]
    target = 20 + 32 + 8 * 26 + sum(full) // 8 + 100000
    eng.profile(True)
    try:
        c, b = eng.compress_to_size(d, CHUNKS, target, return_plan=True)
        import torch
        torch.cuda.synchronize()
        names = {k for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)
    assert [int(v) for v in b] == full
    assert c.numel() == target - 100000 < target
    assert any("k_lis_bits" in k for k in names) and any("k_budget_deal" in k for k in names), sorted(names)
    assert not any("uint64" in k or "unsigned long" in k or "k_make_q_wide" in k for k in names), sorted(names)
    container = host(c)
    check_container(eng, oracle, vol, target, container, [int(v) for v in b], sv)


def test_a_homogeneous_volume_comes_out_even(eng):
    one = plume(np.float32)[:32, :32, :32]
    vol = np.ascontiguousarray(np.tile(one, (2, 2, 2)))
    _, b = eng.compress_to_size(cuda(vol), CHUNKS, vol.size // 8, return_plan=True)
    print("budgets", list(b))
    assert int(b.max()) - int(b.min()) <= 8


# ---- e. a split workspace, a poisoned workspace: in processes of their own ------------------------------------------------

CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from sperr_amd.api import SperrHip
import test_gpu_size as T
eng = SperrHip()
vol = T.plume(np.float32)
d = torch.from_numpy(np.array(vol)).cuda()
eng.profile(True)
c, b = eng.compress_to_size(d, T.CHUNKS, vol.size // 8, return_plan=True)
torch.cuda.synchronize()
counts = {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
eng.profile(False)
back = eng.decompress(c).cpu().numpy()
json.dump({"container": bytes(c.cpu().numpy()).hex(), "budgets": [int(v) for v in b], "counts": counts,
           "back": back.view(np.uint32).tobytes().hex()}, open(sys.argv[2], "w"))
"""


def run_child(tmp_path, env):
    out = tmp_path / "child.json"
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(ROOT), str(out)], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.load(open(out))


def count_of(counts, name):
    return sum(n for k, n in counts.items() if name in k)


@pytest.mark.parametrize("env", [{"SPERR_HIP_ARENA_MAX_MB": "1"}, {"SPERR_HIP_POISON": "0xFF"}], ids=["split", "poison"])
def test_children_make_the_same_container(eng, oracle, tmp_path, env):
    vol = plume(np.float32)
    container, budgets, _ = dealt(eng, vol, vol.size // 8)
    got = run_child(tmp_path, env)
    assert got["budgets"] == budgets
    assert bytes.fromhex(got["container"]) == container
    assert bytes.fromhex(got["back"]) == oracle.decomp_3d(container, True).view(np.uint32).tobytes()
    planes, finals = count_of(got["counts"], "k_plane_table"), count_of(got["counts"], "k_enc_finalize")
    print(env, "k_plane_table", planes, "k_enc_finalize", finals)
    if "SPERR_HIP_ARENA_MAX_MB" in env:   # a chunk per batch, in the survey and in the encode
        assert planes == 8 and finals == 8
    else:
        assert planes == 1 and finals == 1
