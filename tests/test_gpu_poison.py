"""GPU (-m gpu): every device call on a poisoned workspace (SPERR_HIP_POISON).

A call carves its working arrays out of buffers the engine keeps from call to call, over whatever an earlier and
different call left there.  The rule: a kernel may read a workspace word only if this call wrote it or a named clear
covers it.  With SPERR_HIP_POISON=<byte> the engine fills every buffer it holds with that byte before a call carves it
(and what the call allocates or carves again on the way), so a kernel that breaks the rule reads the poison instead of
the zeros of a fresh allocation or the like-shaped residue of the previous test.

Every case runs under 0xFF -- NaN as fp32 and fp64, an all-ones index, but blind to a missing 0xff clear (the decoder's
sign words) -- and under 0x5A, which is blind to neither that nor a missing zero clear.  Every poisoned call, and the
same call with the switch off, is preceded on the same engine by one unpoisoned call of another chunk shape and another
mode (`history`), so that history and poison act together.  A case passes when the poisoned output equals, byte for
byte, the value the existing tests take as truth for the call -- the oracle, the dense call on a packed copy (views,
fields, masked calls), tests/golden/quality_ref.json -- and the same call's output with the switch off.  Where a call
takes out=, the buffer is 0xC3 beforehand and every byte behind the returned length, or outside the written box or
fields, must still be.

Shapes and settings are those of the tests that already prove parity for them (test_gpu_farm.py, test_gpu_parity.py,
test_gpu_value_domains.py, test_gpu_list_patterns.py, test_gpu_slice_patterns.py, test_gpu_workspace_pressure.py,
test_gpu_view.py, test_gpu_fields.py, test_gpu_mask_fill.py, test_gpu_quality.py): no new truth is made here."""
import ctypes as C
import os

import numpy as np
import pytest

import coef_cases as cc
import mask_fill_model as F
import mask_model as M
import quality_cases as qc
import slice_cases as sc
from fields import cached_value_domain_fields, smooth_field, VD_SHAPE
from sperr_amd.farm import split_container
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu
POISON = "SPERR_HIP_POISON"
CAP = "SPERR_HIP_ARENA_MAX_MB"
BYTES = [0xFF, 0x5A]
FILL = 0xC3
C3_WORD = int.from_bytes(bytes([FILL] * 4), "little", signed=True)
_cache = {}


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    e.release()   # (the fills cover what the engine holds: small, whatever earlier files grew)
    e.lib.sperrhip_debug_counter.restype = C.c_ulonglong
    e.lib.sperrhip_debug_counter.argtypes = [C.c_int]
    before = os.environ.get(POISON)
    yield e
    assert os.environ.get(POISON) == before, "a test left the switch behind"
    e.release()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: cached arrays are read-only)


def dev_of(container):
    return cuda(np.frombuffer(container, dtype=np.uint8))


def blob(t):
    """the bytes of a tensor or an array, as they lie when packed"""
    if hasattr(t, "cpu"):
        t = t.contiguous().cpu().numpy()
    return np.ascontiguousarray(t).tobytes()


def sentinel(nbytes):
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


def out_volume(shape, dtype, slack=64):
    """(flat uint8 buffer of 0xC3, a contiguous tensor of `shape` at its start, the bytes behind it)"""
    import torch
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    n = int(np.prod(shape)) * (4 if dt == torch.float32 else 8)
    flat = sentinel(n + slack)
    return flat, flat[:n].view(dt).view(tuple(shape)), flat[n:]


def crop(full, lo, dims):
    return np.ascontiguousarray(full[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])


def span(v):
    v = v.astype(np.float64)
    return float(v.max() - v.min())


def launched(eng, fn):
    """(what fn returns, {kernel name: launches})"""
    import torch
    torch.cuda.synchronize()
    eng.profile(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)


# ---- history: one unpoisoned call of another layout -----------------------------------------------------------------
# Two histories, so that every case has one of another chunk shape AND another mode: a ragged volume in point-wise
# error mode (the outlier coder's buffers, the boxes) for the cases of modes 1 and 2, a fixed-rate one for mode 3.
HISTORY = {3: ((44, 40, 52), (28, 20, 24), 3, 1e-3), 1: ((36, 40, 44), (20, 20, 20), 1, 3.0)}


def history(eng, case_mode, decode):
    """a compression (decode False) or a decode (True) as the call before the one under test, the switch off"""
    assert os.environ.get(POISON) is None
    shape, chunks, mode, q = HISTORY[1 if case_mode == 3 else 3]
    vol = cached(("history", mode), lambda: cuda(turbulence(shape, seed=9)))
    cont = cached(("history_c", mode), lambda: eng.compress(vol, chunks, q, mode=mode).clone())
    if decode:
        eng.decompress(cont, output_float=(mode == 1))
    else:
        eng.compress(vol, chunks, q, mode=mode)


def poisoned(eng, byte, case_mode, decode, call):
    """call() with the switch off and under `byte`, each behind its history -> the poisoned result, seen to equal the
    unpoisoned one.  call() returns a list of bytes objects"""
    history(eng, case_mode, decode)
    off = call()
    history(eng, case_mode, decode)
    with _Env(**{POISON: hex(byte)}):
        on = call()
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a == b, f"output {i} under poison {byte:#x} differs from the same call's with the switch off"
    return on


def test_the_switch_is_off_outside_the_cases():
    assert os.environ.get(POISON) is None


# ---- compress / decompress, fp32 and fp64 ---------------------------------------------------------------------------
def volume(name, dtype):
    def make():
        if name == "one128":
            v = smooth_field((128, 128, 128), seed=31, dtype=np.dtype(dtype).type)
        elif name == "spike":
            v = cached_value_domain_fields(VD_SHAPE, dtype)["spike"]
        else:
            v = turbulence(name, dtype=np.dtype(dtype).type)
        v = np.ascontiguousarray(v)
        v.setflags(write=False)
        return v
    return cached(("vol", name, dtype), make)


def truth(oracle, name, dtype, chunks, mode, q):
    """(the oracle's container, its decode in the volume's precision)"""
    def make():
        want = oracle.comp_3d(volume(name, dtype), chunks, mode, q)
        return want, oracle.decomp_3d(want, dtype == "float32")
    return cached(("truth", name, dtype, chunks, mode, q), make)


def roundtrip(eng, oracle, byte, name, dtype, chunks, mode, q):
    """compress into a 0xC3 buffer and decode into one, both poisoned, both against the oracle"""
    v = volume(name, dtype)
    want, ref = truth(oracle, name, dtype, chunks, mode, q)
    dv = cuda(v)
    cap = eng.max_compressed_size(v.shape, chunks, q, mode)

    def enc():
        buf = sentinel(cap + 64)
        got = eng.compress(dv, chunks, q, out=buf, mode=mode)
        assert got.data_ptr() == buf.data_ptr()
        return [blob(got), blob(buf[got.numel():])]

    got, tail = poisoned(eng, byte, mode, False, enc)
    assert got == want, "the container differs from the oracle's"
    assert tail == bytes([FILL]) * len(tail), "bytes behind the container were written"
    dev = dev_of(want)

    def dec():
        flat, out, rest = out_volume(v.shape, dtype)
        assert eng.decompress(dev, output_float=(dtype == "float32"), out=out) is out
        return [blob(out), blob(rest)]

    back, tail = poisoned(eng, byte, mode, True, dec)
    assert back == ref.tobytes(), "the decode differs from the oracle's"
    assert tail == bytes([FILL]) * len(tail), "bytes behind the volume were written"
    return want


# (z, y, x) / chunks / mode / quality, as tests/test_gpu_farm.py CASES has them
ROUNDTRIPS = {
    "ragged_rate": ((96, 80, 72), (32, 32, 32), 1, 2.0),      # four chunk shapes, k_lis_mx, groups side by side
    "psnr": ((50, 64, 72), (20, 30, 40), 2, 70.0),            # q search, stream lengths unknown beforehand
    "pwe": ((72, 48, 40), (24, 24, 20), 3, 1e-3),             # outlier coder both ways, pweBox, decBox, outlDec
}


@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", sorted(ROUNDTRIPS))
def test_compress_decompress(eng, oracle, case, dtype, byte):
    shape, chunks, mode, q = ROUNDTRIPS[case]
    roundtrip(eng, oracle, byte, shape, dtype, chunks, mode, q)


@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_one_128_cube_chunk(eng, oracle, dtype, byte):
    """one 128^3 chunk at 2 bpp: the fused second level (floor 96), k_pix_turn (floor 64), k_lis_hi / _l0 / _l1 / _l2,
    the refinement planes in the coefficient array"""
    roundtrip(eng, oracle, byte, "one128", dtype, (128, 128, 128), 1, 2.0)


@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_64_bit_retry(eng, oracle, dtype, byte):
    """tests/test_gpu_value_domains.py's spike at 24 bpp, one chunk: 53 bit planes, so the fixed-rate encoder codes it
    with 32-bit coefficients first and again with 64-bit ones (wideScratch, bb.vals)"""
    chunks = VD_SHAPE[::-1]
    redo0 = eng.lib.sperrhip_debug_counter(0)
    want = roundtrip(eng, oracle, byte, "spike", dtype, chunks, 1, 24.0)
    assert [p[17] for p in split_container(want)[3]] == [53]
    assert eng.lib.sperrhip_debug_counter(0) - redo0 >= 2, "the chunk buffer was not transformed again"


# ---- the coders alone ----------------------------------------------------------------------------------------------
STAGE_3D = ("checker8", "stagger8_one")   # the first two of coef_cases.CASES (the cheapest first) that CONDITIONS names
# slice_cases: the smallest shape is FLAT (9 x 2048); of its entries a list case and a type-I case
STAGE_2D = (("checker2", sc.FLAT), ("i_dense", sc.FLAT))


def stage(eng, byte, coef, sign, wide, shape, enc_o, dec_o, enc_e, dec_e):
    dcoef = cuda(coef.view(np.int64) if wide else coef.astype(np.uint32).view(np.int32))
    dsign = cuda(sign.view(np.int64))
    want = enc_o(coef, sign, 0)
    got, = poisoned(eng, byte, 1, False, lambda: [enc_e(dcoef, dsign, 0)])
    assert got == want, "the stream differs from the oracle's"
    for cut in (len(want), 9 + (len(want) - 9) // 2):
        c0, s0 = dec_o(want[:cut], shape)
        c1, s1 = poisoned(eng, byte, 1, True, lambda: [x.tobytes() for x in dec_e(want[:cut], shape)])
        assert c1 == np.ascontiguousarray(c0, dtype=np.uint64).tobytes(), cut
        assert s1 == np.ascontiguousarray(s0, dtype=np.uint64).tobytes(), cut


@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("name", STAGE_3D)
def test_speck3d_stage(eng, oracle, name, byte):
    assert [n for n in cc.CASES if any(c[0] == n for c in cc.CONDITIONS)][:2] == list(STAGE_3D)
    coef, sign, wide = cc.case(name, cc.SHAPE)
    stage(eng, byte, coef, sign, wide, cc.SHAPE, oracle.speck3d_encode, oracle.speck3d_decode, eng.speck3d_encode,
          eng.speck3d_decode)


@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("name,shape", STAGE_2D, ids=[n for n, _ in STAGE_2D])
def test_speck2d_stage(eng, oracle, name, shape, byte):
    assert int(np.prod(shape)) == min(int(np.prod(s)) for _, s in sc.ALL_CASES) and (name, shape) in sc.ALL_CASES
    coef, sign, wide = sc.case(name, shape)
    stage(eng, byte, coef, sign, wide, shape, oracle.speck2d_encode, oracle.speck2d_decode, eng.speck2d_encode,
          eng.speck2d_decode)


@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("shape", [(33, 17, 9), (128, 128, 128)], ids=["33x17x9", "128cube"])
def test_dwt3d_both_ways(eng, oracle, shape, byte):
    """(tests/test_gpu_parity.py: bit-exact against the oracle's transform, both ways)"""
    v = cached(("dwt", shape), lambda: turbulence(shape, dtype=np.float64))
    fwd = cached(("dwt_fwd", shape), lambda: oracle.dwt3d(v))
    inv = cached(("dwt_inv", shape), lambda: oracle.idwt3d(fwd))
    got, = poisoned(eng, byte, 1, False, lambda: [blob(eng.dwt3d(cuda(v)))])
    assert got == np.ascontiguousarray(fwd).tobytes()
    got, = poisoned(eng, byte, 1, True, lambda: [blob(eng.dwt3d(cuda(fwd), inverse=True))])
    assert got == np.ascontiguousarray(inv).tobytes()


# ---- slices ---------------------------------------------------------------------------------------------------------
SLICE_YX, SLICE_MODE, SLICE_Q = (75, 100), 2, 90.0   # 100 x 75


@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_slices_one_and_three(eng, oracle, dtype, byte):
    of = dtype == "float32"
    imgs = cached(("imgs", dtype), lambda: np.stack([turbulence((1,) + SLICE_YX, seed=200 + s, dtype=np.dtype(dtype).type)[0]
                                                     for s in range(3)]))
    wants = cached(("imgs_c", dtype), lambda: [oracle.comp_2d(i, SLICE_MODE, SLICE_Q, False) for i in imgs])
    refs = cached(("imgs_d", dtype), lambda: [oracle.decomp_2d(w, SLICE_YX, of) for w in wants])
    d0 = cuda(imgs[0])
    got, = poisoned(eng, byte, SLICE_MODE, False, lambda: [blob(eng.compress_2d(d0, SLICE_Q, mode=SLICE_MODE))])
    assert got == wants[0]
    s0 = dev_of(wants[0])
    got, = poisoned(eng, byte, SLICE_MODE, True, lambda: [blob(eng.decompress_2d(s0, SLICE_YX, output_float=of))])
    assert got == refs[0].tobytes()
    dall = cuda(imgs)
    cap = eng.max_compressed_size_2d_batch(3, SLICE_YX, SLICE_Q, SLICE_MODE)

    def enc():
        buf = sentinel(cap + 64)
        parts = eng.compress_2d_batch(dall, SLICE_Q, mode=SLICE_MODE, out=buf)
        assert parts[0].data_ptr() == buf.data_ptr()
        return [blob(p) for p in parts] + [blob(buf[sum(p.numel() for p in parts):])]

    *parts, tail = poisoned(eng, byte, SLICE_MODE, False, enc)
    assert parts == wants and tail == bytes([FILL]) * len(tail)
    streams = [dev_of(w) for w in wants]

    def dec():
        flat, out, rest = out_volume((3,) + SLICE_YX, dtype)
        eng.decompress_2d_batch(streams, SLICE_YX, output_float=of, out=out)
        return [blob(out), blob(rest)]

    back, tail = poisoned(eng, byte, SLICE_MODE, True, dec)
    assert back == b"".join(r.tobytes() for r in refs) and tail == bytes([FILL]) * len(tail)


# ---- a batch of volumes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", BYTES, ids=hex)
def test_batch_of_three_volumes(eng, oracle, byte):
    """3 x (40, 48, 56) in 24^3 chunks: the volumes' chunks share the shape groups"""
    shape, chunks, q = (40, 48, 56), (24, 24, 24), 2.5
    vols = cached("batch_v", lambda: np.stack([turbulence(shape, seed=50 + k) for k in range(3)]))
    wants = cached("batch_c", lambda: [oracle.comp_3d(v, chunks, 1, q) for v in vols])
    refs = cached("batch_d", lambda: [oracle.decomp_3d(w, True) for w in wants])
    dv = cuda(vols)
    cap = eng.max_compressed_size_batch(3, shape, chunks, q, 1)

    def enc():
        buf = sentinel(cap + 64)
        parts = eng.compress_batch(dv, chunks, q, out=buf)
        assert parts[0].data_ptr() == buf.data_ptr()
        return [blob(p) for p in parts] + [blob(buf[sum(p.numel() for p in parts):])]

    *parts, tail = poisoned(eng, byte, 1, False, enc)
    assert parts == wants and tail == bytes([FILL]) * len(tail)
    conts = [dev_of(w) for w in wants]

    def dec():
        flat, out, rest = out_volume((3,) + shape, "float32")
        eng.decompress_batch(conts, output_float=True, out=out)
        return [blob(out), blob(rest)]

    back, tail = poisoned(eng, byte, 1, True, dec)
    assert back == b"".join(r.tobytes() for r in refs) and tail == bytes([FILL]) * len(tail)


# ---- the refill between batches of workspace ------------------------------------------------------------------------
@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("mode,q", [(1, 2.0), (3, 1e-3)])
def test_ragged_volume_under_the_arena_cap(eng, oracle, mode, q, byte):
    """tests/test_gpu_workspace_pressure.py::test_b3_ragged_volume under cap 1: (72, 80, 100) in 32^3 chunks, 12 chunks in
    8 shape groups, one chunk per batch both ways -- the arena is carved, and under the switch filled, twelve times a
    call; the decoder's deferred groups drain in between"""
    v = cached("b3", lambda: turbulence((72, 80, 100)))
    chunks = (32, 32, 32)
    if mode == 3:
        q = q * span(v)
    want = cached(("b3_c", mode), lambda: oracle.comp_3d(v, chunks, mode, q))
    ref = cached(("b3_d", mode), lambda: oracle.decomp_3d(want, True))
    dv, dev = cuda(v), dev_of(want)

    def capped(fn):
        def run():
            eng.release()   # (the arena really is as small as the cap says: _Cap of the pressure file)
            with _Env(**{CAP: 1}):
                out, names = launched(eng, fn)
            eng.release()
            return out, names
        return run

    enc = capped(lambda: blob(eng.compress(dv, chunks, q, mode=mode)))
    dec = capped(lambda: blob(eng.decompress(dev, output_float=True)))
    counts = {}

    def call(run, witness, tag):
        def go():
            out, names = run()
            counts[tag] = names.get(witness, 0)
            return [out]
        return go

    got, = poisoned(eng, byte, mode, False, call(enc, "k_mean_finalize<T>", "enc"))
    assert got == want
    back, = poisoned(eng, byte, mode, True, call(dec, "k_dec_header", "dec"))
    assert back == ref.tobytes()
    assert counts == {"enc": 12, "dec": 12}, counts   # (the pressure file's witnesses: a batch per chunk, eleven refills)


# ---- box, level, portion, boxes, truncate ---------------------------------------------------------------------------
BOX_LO, BOX_DIMS = (5, 9, 3), (61, 70, 80)   # (x, y, z) of the (z, y, x) = (96, 80, 72) volume: meets all 12 chunks


@pytest.mark.parametrize("byte", BYTES, ids=hex)
def test_windows_of_the_ragged_container(eng, oracle, byte):
    shape, chunks, mode, q = ROUNDTRIPS["ragged_rate"]
    want, ref = truth(oracle, shape, "float32", chunks, mode, q)
    dev = dev_of(want)
    zyx = tuple(reversed(BOX_DIMS))

    def box():
        flat, out, rest = out_volume(zyx, "float32")
        eng.decompress_box(dev, BOX_LO, BOX_DIMS, output_float=True, out=out)
        return [blob(out), blob(rest)]

    got, tail = poisoned(eng, byte, mode, True, box)
    assert got == crop(ref, BOX_LO, BOX_DIMS).tobytes() and tail == bytes([FILL]) * len(tail)

    part = cached("trunc37", lambda: oracle.trunc_3d(want, 37))
    part_ref = cached("trunc37_d", lambda: oracle.decomp_3d(part, True))

    def portion():
        flat, out, rest = out_volume(shape, "float32")
        eng.decompress(dev, output_float=True, out=out, pct=37)
        return [blob(out), blob(rest)]

    got, tail = poisoned(eng, byte, mode, True, portion)
    assert got == part_ref.tobytes() and tail == bytes([FILL]) * len(tail)

    def trunc():
        buf = sentinel(len(want) + 64)
        t = eng.truncate(dev, 37, out=buf)
        assert t.data_ptr() == buf.data_ptr()
        return [blob(t), blob(buf[t.numel():])]

    got, tail = poisoned(eng, byte, mode, True, trunc)
    assert got == part and tail == bytes([FILL]) * len(tail)

    # two entries out of one container whose boxes share chunks: the staged form (boxesStage)
    los, dims = [(5, 9, 3), (20, 30, 10)], (40, 35, 50)
    plan = eng.boxes_plan(shape, [chunks], los, dims, which=[0, 0])
    assert plan["staged"], plan
    bz = tuple(reversed(dims))

    def boxes():
        flat, out, rest = out_volume((2,) + bz, "float32")
        eng.decompress_boxes([dev], los, dims, which=[0, 0], output_float=True, out=out)
        return [blob(out), blob(rest)]

    got, tail = poisoned(eng, byte, mode, True, boxes)
    assert got == b"".join(crop(ref, lo, dims).tobytes() for lo in los) and tail == bytes([FILL]) * len(tail)


@pytest.mark.parametrize("byte", BYTES, ids=hex)
def test_levels_of_a_dyadic_container(eng, oracle, byte):
    """(64, 64, 64) in 32^3 chunks at 4 bpp (test_gpu_farm.py): every level of its hierarchy, as fp64"""
    v = cached("lv_v", lambda: turbulence((64, 64, 64)))
    want = cached("lv_c", lambda: oracle.comp_3d(v, (32, 32, 32), 1, 4.0))
    levels = cached("lv_l", lambda: oracle.decomp_3d_multi_res(want)[1])
    assert len(levels) > 1 and len(eng.multires_levels((64, 64, 64), (32, 32, 32))) == len(levels)
    dev = dev_of(want)
    for h, lv in enumerate(levels):
        def level():
            flat, out, rest = out_volume(lv.shape, "float64")
            eng.decompress_level(dev, h, output_float=False, out=out)
            return [blob(out), blob(rest)]

        got, tail = poisoned(eng, byte, 1, True, level)
        assert got == np.ascontiguousarray(lv).tobytes(), h
        assert tail == bytes([FILL]) * len(tail), h


# ---- views and interleaved fields -----------------------------------------------------------------------------------
F_SHAPE, F_CHUNKS, F_Q = (30, 44, 37), (32, 32, 32), 2.5   # tests/test_gpu_fields.py
LO, HI = (1, 2, 3), (1, 2, 4)                              # ghost cells (z, y, x): tests/test_gpu_view.py halo_parent


def three_fields():
    t = turbulence(F_SHAPE, dtype=np.float64)
    return np.stack([t.astype(np.float32), (100.0 * t).astype(np.float32), np.full(F_SHAPE, 2.75, dtype=np.float32)])


def halo(inner_shape, tail=()):
    """(flat 0xC3 buffer, its fp32 tensor with ghost cells around `inner_shape` (+ tail dims), the interior view)"""
    import torch
    full = tuple(a + n + b for a, n, b in zip(LO, inner_shape, HI)) + tuple(tail)
    flat = sentinel(int(np.prod(full)) * 4)
    whole = flat.view(torch.float32).view(full)
    return flat, whole, whole[tuple(slice(a, a + n) for a, n in zip(LO, inner_shape))]


@pytest.mark.parametrize("byte", BYTES, ids=hex)
def test_strided_view_in_and_out(eng, oracle, byte):
    """the interior of an array with ghost cells: the container is the dense call's on the packed copy and the
    oracle's; the decode goes into the interior of another and the ghost cells stay 0xC3"""
    import torch
    v = cached("fields_v", three_fields)[0]
    want = cached("view_c", lambda: oracle.comp_3d(v, F_CHUNKS, 1, F_Q))
    ref = cached("view_d", lambda: oracle.decomp_3d(want, True))
    flat, whole, w = halo(F_SHAPE)
    w.copy_(torch.from_numpy(v).cuda())
    assert not w.is_contiguous()
    before = flat.clone()
    got, = poisoned(eng, byte, 1, False, lambda: [blob(eng.compress(w, F_CHUNKS, F_Q))])
    assert got == blob(eng.compress(w.contiguous(), F_CHUNKS, F_Q)) and got == want
    assert bool((flat == before).all()), "compress wrote to its source"
    dev = dev_of(want)

    def dec():
        flat, whole, out = halo(F_SHAPE)
        assert eng.decompress(dev, output_float=True, out=out) is out
        got = blob(out)
        out.view(torch.int32).fill_(C3_WORD)   # (the interior back to 0xC3: what is left is the ghost cells)
        return [got, blob(flat)]

    back, rest = poisoned(eng, byte, 1, True, dec)
    assert back == ref.tobytes()
    assert rest == bytes([FILL]) * len(rest), "ghost cells were written"


@pytest.mark.parametrize("byte", BYTES, ids=hex)
def test_interleaved_fields(eng, oracle, byte):
    """three fields, channels last, inside ghost cells: container f is the oracle's of the packed field f; the decode
    goes into fields 1..3 of a four-field record inside ghost cells, field 0 and the ghost cells stay 0xC3"""
    import torch
    fields = cached("fields_v", three_fields)
    wants = cached("fields_c", lambda: [oracle.comp_3d(f, F_CHUNKS, 1, F_Q) for f in fields])
    refs = cached("fields_d", lambda: [oracle.decomp_3d(w, True) for w in wants])
    flat, whole, inter = halo(F_SHAPE, tail=(3,))
    inter.copy_(torch.from_numpy(np.ascontiguousarray(fields.transpose(1, 2, 3, 0))).cuda())
    before = flat.clone()
    cap = eng.max_compressed_size_batch(3, F_SHAPE, F_CHUNKS, F_Q, 1)

    def enc():
        buf = sentinel(cap + 64)
        parts = eng.compress_fields(inter, F_CHUNKS, F_Q, out=buf)
        assert parts[0].data_ptr() == buf.data_ptr()
        return [blob(p) for p in parts] + [blob(buf[sum(p.numel() for p in parts):])]

    *parts, tail = poisoned(eng, byte, 1, False, enc)
    assert parts == wants and tail == bytes([FILL]) * len(tail)
    assert bool((flat == before).all()), "compress_fields wrote to its source"
    conts = [dev_of(w) for w in wants]

    def dec():
        flat, whole, rec = halo(F_SHAPE, tail=(4,))
        out = rec[..., 1:4]
        assert eng.decompress_fields(conts, out=out) is out
        got = [blob(out[..., f]) for f in range(3)]
        out.view(torch.int32).fill_(C3_WORD)   # (the three fields back to 0xC3: what is left is field 0 and the ghost cells)
        return got + [blob(flat)]

    *back, rest = poisoned(eng, byte, 1, True, dec)
    assert back == [r.tobytes() for r in refs]
    assert rest == bytes([FILL]) * len(rest), "field 0 or the ghost cells were written"


# ---- missing values -------------------------------------------------------------------------------------------------
MASK_ZYX, MASK_CHUNKS, MASK_Q = (48, 64, 56), (16, 16, 16), 2.5   # 56 x 64 x 48; chunks and rate: test_gpu_mask_fill.py


def masked_volume():
    v = turbulence(MASK_ZYX)
    mask = M.ball_mask(MASK_ZYX, 20)
    v[mask] = np.nan
    return v, mask, F.smooth_filled(v, mask)


@pytest.mark.parametrize("byte", BYTES, ids=hex)
def test_masked_calls(eng, oracle, byte):
    """a ball of NaNs: the container is the oracle's of the model's smooth in-fill (and the dense call's on it), the mask
    stream the model's; the decode is the oracle's with the value at the ball; the figures are quality()'s on the
    compacted arrays; mask_make and mask_apply against the model"""
    import torch
    v, mask, filled = cached("masked", masked_volume)
    want = cached("masked_c", lambda: oracle.comp_3d(filled, MASK_CHUNKS, 1, MASK_Q))
    ref = cached("masked_d", lambda: oracle.decomp_3d(want, True))
    dv = cuda(v)
    cont, stream = poisoned(eng, byte, 1, False,
                            lambda: [blob(t) for t in eng.compress_masked(dv, MASK_CHUNKS, MASK_Q, fill="smooth")])
    assert stream == M.stream(mask) and cont == want
    assert cont == blob(eng.compress(cuda(filled), MASK_CHUNKS, MASK_Q))
    dcont = dev_of(want)
    dmask = torch.empty(len(stream) + 8, dtype=torch.uint8, device="cuda")
    dmask = dmask[(-dmask.data_ptr()) % 8:][:len(stream)]
    dmask.copy_(torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()))
    holed = ref.copy()
    holed[mask] = np.float32(1e20)

    def dec():
        flat, out, rest = out_volume(MASK_ZYX, "float32")
        eng.decompress_masked(dcont, dmask, 1e20, output_float=True, out=out)
        return [blob(out), blob(rest)]

    back, tail = poisoned(eng, byte, 1, True, dec)
    assert back == holed.tobytes() and tail == bytes([FILL]) * len(tail)

    recon = cuda(holed)
    fig = lambda f: np.array([f.rmse, f.linfty, f.psnr, f.min, f.max, f.mean, f.var, f.mse]).tobytes()
    got, = poisoned(eng, byte, 1, True, lambda: [fig(eng.quality_masked(dv, recon, dmask))])
    keep = torch.from_numpy(~mask).cuda()
    assert got == fig(eng.quality(dv[keep].contiguous(), recon[keep].contiguous()))

    def make():
        flat, out, rest = out_volume(MASK_ZYX, "float32")
        m, nmiss = eng.mask_make(dv, fill="smooth", filled_out=out)
        return [blob(m), blob(out), blob(rest), str(nmiss).encode()]

    m, fl, tail, nmiss = poisoned(eng, byte, 1, False, make)
    assert m == M.stream(mask) and fl == filled.tobytes() and int(nmiss) == int(mask.sum())
    assert tail == bytes([FILL]) * len(tail)

    got, = poisoned(eng, byte, 1, True, lambda: [blob(eng.mask_apply(cuda(ref), dmask, 1e20))])
    assert got == holed.tobytes()


# ---- quality figures ------------------------------------------------------------------------------------------------
BITWISE = ("rmse", "linfty", "mean", "var", "mse")   # tests/test_gpu_quality.py: psnr within 8 ulp, min and max by value


def check_quality(q, rec, what):
    dt = qc.DTYPES[rec["dtype"]]
    for f in BITWISE:
        assert qc.to_hex(dt(getattr(q, f))) == format(int(rec[f], 16), "x"), (what, f)
    for f in ("min", "max"):
        assert dt(getattr(q, f)) == qc.from_hex(rec[f], dt), (what, f)
    assert qc.ulp_distance(dt(q.psnr), qc.from_hex(rec["psnr"], dt), dt) <= 8, (what, "psnr")


@pytest.mark.parametrize("byte", BYTES, ids=hex)
@pytest.mark.parametrize("key", ["f32", "f64"])
def test_quality_and_quality_batch(eng, key, byte):
    """size_57349 (three blocks of 16384, one of 8192, a tail of 5) and the batch of three odd volumes, against
    tests/golden/quality_ref.json: the partial sums"""
    fx = cached("qfx", qc.load_fixture)
    name = f"size_57349_{key}"
    a, b = qc.cases()[name]()
    da, db = cuda(a), cuda(b)
    figs = lambda q: np.array([getattr(q, f) for f in qc.FIGURES]).tobytes()
    kept = {}

    def one():
        kept["q"] = eng.quality(da, db)
        return [figs(kept["q"])]

    poisoned(eng, byte, 1, True, one)
    check_quality(kept["q"], fx[name], name)
    a3, b3 = qc.batch(3, qc.N_BATCH3, qc.DTYPES[key], 31)
    da3, db3 = cuda(a3), cuda(b3)

    def three():
        kept["qs"] = eng.quality_batch(da3, db3)
        return [figs(q) for q in kept["qs"]]

    poisoned(eng, byte, 1, True, three)
    for v, q in enumerate(kept["qs"]):
        check_quality(q, fx[f"batch3_v{v}_{key}"], f"batch3 v{v}")


# ---- the chunk farm: the workers' own engines -----------------------------------------------------------------------
@pytest.mark.parametrize("byte", BYTES, ids=hex)
def test_farm_with_two_workers_on_one_device(eng, oracle, byte):
    """(64, 64, 64) in 32^3 chunks at 4 bpp on devices [0, 0] (test_gpu_farm.py); the history goes through the farm too,
    so that the workers' engines hold another layout"""
    v = cached("lv_v", lambda: turbulence((64, 64, 64)))
    want = cached("lv_c", lambda: oracle.comp_3d(v, (32, 32, 32), 1, 4.0))
    ref = cached("lv_d", lambda: oracle.decomp_3d(want, True))
    hv = cached("farm_h", lambda: turbulence((44, 40, 52), seed=9))
    ht = 1e-3 * span(hv)
    hc = cached("farm_hc", lambda: oracle.comp_3d(hv, (28, 20, 24), 3, ht))

    def enc():
        assert eng.comp_3d_farm(hv, (28, 20, 24), 3, ht, devices=[0, 0]) == hc
        return [eng.comp_3d_farm(v, (32, 32, 32), 1, 4.0, devices=[0, 0])]

    def dec():
        eng.decomp_3d_farm(hc, True, devices=[0, 0])
        return [eng.decomp_3d_farm(want, True, devices=[0, 0]).tobytes()]

    got, = poisoned(eng, byte, 1, False, enc)
    assert got == want
    back, = poisoned(eng, byte, 1, True, dec)
    assert back == ref.tobytes()


# ---- the switch off adds no launches --------------------------------------------------------------------------------
# Launches of compress() and of decompress(output_float=True) of the fp32 128^3 case above, one chunk at 2 bpp, counted
# by the engine's profiler on an MI355X with the library of commit 60394e6 ("Cut xform.hip into conditioner, per-axis
# and fused lifting units"), the parent of the commit that added the switch.
PARENT_LAUNCHES = {"compress": 114, "decompress": 271}


def test_switch_off_adds_no_launches(eng, oracle):
    assert os.environ.get(POISON) is None
    want, _ = truth(oracle, "one128", "float32", (128, 128, 128), 1, 2.0)
    dv, dev = cuda(volume("one128", "float32")), dev_of(want)
    eng.compress(dv, (128, 128, 128), 2.0)   # (plans and buffers are made: the counted calls allocate nothing)
    eng.decompress(dev, output_float=True)
    _, enc = launched(eng, lambda: eng.compress(dv, (128, 128, 128), 2.0))
    _, dec = launched(eng, lambda: eng.decompress(dev, output_float=True))
    print("compress", sum(enc.values()), "decompress", sum(dec.values()))
    assert sum(enc.values()) == PARENT_LAUNCHES["compress"], sorted(enc.items())
    assert sum(dec.values()) == PARENT_LAUNCHES["decompress"], sorted(dec.items())
