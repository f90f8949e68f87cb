"""GPU: calls whose shape groups need more than one batch of workspace (encode_group, encode.hip / decode_group, decode.hip).

A group is coded in batches of B = min(group size, max(1, budget / bytes per chunk), 256) chunks.  With B below the
group size the batch loops run more than once: the arena is carved again for every batch, chunk ids come from
refs[b0 + i], sub-batches start at b0 + done, side-by-side encoding falls back, deferred groups drain when the arena is
full, the point-wise-error stage waits for the previous batch's, and the 64-bit retry lands in a later batch.  This file
gets B below the group size in both ways there are:

  A  more than 256 chunks of one transformed shape (9^3 chunks: one transform level, the lifting kernels and the real
     coder), nothing in the environment touched;
  B  SPERR_HIP_ARENA_MAX_MB around the calls under test, on 32^3 chunks (the table list kernels), 64^3 chunks (fused
     head, brick, compact box, fused second level) and a ragged volume (non-dyadic groups through k_lis_mx, deferral).
     The engine is released before a capped call, so its arena really is as small as the cap says and Arena::take's
     bounds check guards every carve, and again after it.

Every comparison is against the CPU oracle: container bytes, and decoded bit patterns as fp32 and as fp64.

Workspace per chunk, in MiB, as SPERR_HIP_ARENA_DEBUG=1 printed it on an MI355X (encoder at 2 bpp / a PSNR target / a
point-wise tolerance; decoder of those containers; the decoder adds 1 MiB to every batch):
    9^3     encoder 0.19 / 0.20 / 0.21     decoder  7.06 /  7.06 /  7.07
    32^3    encoder 0.84 / 1.12 / 1.36     decoder  7.51 /  7.58 /  7.78
    64^3    encoder 5.07 / 7.38 / 9.24     decoder 11.01 / 12.39 / 14.00
(the decoder's 7.02 MiB of queues per chunk do not depend on the shape; the encoder's stream grows with the rate, by
rate x samples / 8 bytes: 64^3 at 24 bpp 5.8, at 40 bpp 6.3 MiB, and the launch counts at those rates are three
batches' indeed).  The caps that rest on them:
    cap 1   every shape above needs more than half a MiB per chunk in either direction: one chunk per batch
    64^3, three chunks per batch (3 + 3 + 2): encoder at a fixed rate 19 (three chunks at 40 bpp take 18.8, four at
    2 bpp 20.3), encoder with a tolerance 32 (27.7 to 37.0), decoder of a fixed-rate container 38 (33.0 to 44.0),
    decoder of a tolerance container 48 (42.0 to 56.0)

Witnesses that the split happened, from launch counts (eng.profile): k_mean_finalize runs once per encoder batch (twice
where a 64-bit retry transforms the batch again, so it is read at 2 bpp), k_dec_header once per decoder sub-batch (the
profiler sees the sub-batch threads' launches).
  * Encoder, B1, B2: capped at least three times the uncapped count (1), and exactly the batches expected (8; 3).
  * Decoder, B1, B2: an uncapped call decodes its 8 chunks as ONE batch cut into four sub-batches (pick_sub_batches),
    a batch of fewer than four chunks has one sub-batch -- so no cap can triple k_dec_header (8 chunks: at most 8
    against 4).  In batches the condition holds, 8 and 3 against 1, and the test asserts the counts that say so:
    uncapped 4, capped exactly 8 (B1) and 3 (B2).
  * B3: the ragged volume has 12 chunks in 8 groups, none with more than two chunks, so no group can triple either.
    Uncapped every group is one batch (8); under cap 1 every chunk is (12), which says that each of the four groups
    of two chunks was split.  Asserted for both directions.
  * A1, decoder: 343 chunks launch exactly twice what 64 chunks of the shape do (batches of 256 and 87 with three
    sub-batches each, against one batch with three).
  * A1, encoder: at a fixed rate a group of 64 to 512 chunks is cut into four parts that are coded side by side
    (group_chunks), so 343 chunks are four groups of 85 or 86 and 64 chunks four groups of 16: no batch loop runs
    twice, and the counts are equal.  The other two modes have no parts: there 343 chunks are batches of 256 and 87,
    and the PSNR case asserts exactly twice the 64-chunk count.  The fixed-rate encoder's batch loop is witnessed by
    B1 to B3 (fewer than 64 chunks: one part), and without the cap by 729 chunks (beyond 512 there are no parts
    either: batches of 256, 256 and 217, exactly three times the count of a 27-chunk volume).
Parity only, no counter: drain() (A2, B3: deferred groups beside a group that is split, and the drain when the arena has
no room), the side-by-side fallback (B3 at a fixed rate), pwe_stage_begin's wait for the previous batch (every
tolerance case), the decode fronts of B4 and k_lis_mx's workgroup budget."""
import ctypes as C
import os

import numpy as np
import pytest

from fields import ramp_field, smooth_field
from sperr_amd.farm import chunk_grid, split_container
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu
CAP = "SPERR_HIP_ARENA_MAX_MB"
ENC_RATE_64, ENC_PWE_64, DEC_RATE_64, DEC_PWE_64 = 19, 32, 38, 48   # three 64^3 chunks per batch, see above
ENC_WITNESS, DEC_WITNESS = "k_mean_finalize<T>", "k_dec_header"
C9, C32, C64 = (9, 9, 9), (32, 32, 32), (64, 64, 64)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    e.lib.sperrhip_debug_counter.restype = C.c_ulonglong
    e.lib.sperrhip_debug_counter.argtypes = [C.c_int]
    before = os.environ.get(CAP)
    yield e
    assert os.environ.get(CAP) == before, "a test left the cap behind"
    e.release()


class _Cap:
    """SPERR_HIP_ARENA_MAX_MB = mb around the calls inside (the library reads it per call), the engine's memory given
    back before and after; mb None: nothing is touched"""

    def __init__(self, eng, mb):
        self.eng, self.mb = eng, mb

    def __enter__(self):
        if self.mb is None:
            return self
        self.old = os.environ.get(CAP)
        self.eng.release()
        os.environ[CAP] = str(self.mb)
        return self

    def __exit__(self, *exc):
        if self.mb is None:
            return False
        if self.old is None:
            os.environ.pop(CAP, None)
        else:
            os.environ[CAP] = self.old
        self.eng.release()
        return False


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the bank's arrays are read-only)


def dev_of(container):
    return cuda(np.frombuffer(container, dtype=np.uint8).copy())


def host(t):
    return bytes(t.cpu().numpy())


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want):
    if hasattr(got, "cpu"):
        got = got.cpu().numpy()
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


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


# ---- the fields, made once per module, and what the oracle makes of them ------------------------------------------
def _wide_128():
    """eight 64^3 chunks (x fastest), the data of test_gpu_fused_head.py's wide_retry_64 extended: smooth noise, the
    ramp as chunk 4 -- batches of three put it into the second batch --, and as chunks 1 and 5 turbulence, which
    alone asks for the 64-bit retry at 24 bpp (test_gpu_batch.py::test_wide_retry_of_some_chunks); at 40 bpp all do"""
    v = np.empty((128, 128, 128), dtype=np.float32)
    for i, (x0, lx, y0, ly, z0, lz) in enumerate(chunk_grid((128, 128, 128), C64)):
        piece = (ramp_field((64, 64, 64)) if i == 4 else turbulence((64, 64, 64), seed=30 + i) if i in WIDE_AT_24 else
                 smooth_field((64, 64, 64), seed=41 + i))
        v[z0:z0 + lz, y0:y0 + ly, x0:x0 + lx] = piece
    return v


WIDE_AT_24 = (1, 5)
_MAKE = {
    "a1_f32": lambda: turbulence((63, 63, 63)),
    "a1_f64": lambda: turbulence((63, 63, 63), seed=43, dtype=np.float64),
    "a1_64": lambda: turbulence((36, 36, 36)),
    "a1_729": lambda: turbulence((81, 81, 81), seed=47),
    "a1_27": lambda: turbulence((27, 27, 27)),
    "a2": lambda: turbulence((66, 63, 70), seed=44),
    "a3_0": lambda: turbulence((45, 45, 54), seed=45),
    "a3_1": lambda: turbulence((45, 45, 54), seed=46),
    "b1": lambda: turbulence((64, 64, 64)),
    "b2": lambda: smooth_field((128, 128, 128), seed=31),
    "b2_wide": _wide_128,
    "b2_other1": lambda: smooth_field((128, 128, 128), seed=32),
    "b2_other2": lambda: smooth_field((128, 128, 128), seed=33, passes=2),
    "b3": lambda: turbulence((72, 80, 100)),
    "b5": lambda: smooth_field((64, 64, 64), seed=41),
}


class Bank:
    """fields by name, and the oracle's containers and decodes of them, each made once and handed out read-only"""

    def __init__(self, oracle):
        self.oracle, self.kept = oracle, {}

    def get(self, key, make):
        if key not in self.kept:
            v = make()
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            self.kept[key] = v
        return self.kept[key]

    def field(self, name):
        return self.get(("f", name), _MAKE[name])

    def container(self, name, ch, mode, q):
        return self.get(("c", name, ch, mode, q), lambda: self.oracle.comp_3d(self.field(name), ch, mode, q))

    def decoded(self, container, of):
        return self.get(("d", container, of), lambda: self.oracle.decomp_3d(container, of))

    def levels(self, container):
        return self.get(("l", container), lambda: self.oracle.decomp_3d_multi_res(container))


@pytest.fixture(scope="module")
def bank(oracle):
    return Bank(oracle)


def roundtrip(eng, bank, name, ch, mode, q, enc_cap=None, dec_cap=None):
    """compress field `name` (under enc_cap) and decode the oracle's container of it as fp32 and fp64 (under dec_cap),
    all against the oracle; -> (the compress call's launches, the fp32 decode's)"""
    v = bank.field(name)
    want = bank.container(name, ch, mode, q)
    dv = cuda(v)
    with _Cap(eng, enc_cap):
        got, enc = launched(eng, lambda: host(eng.compress(dv, ch, q, mode=mode)))
    assert got == want, (name, mode, q, enc_cap, "container differs from the oracle's")
    dev = dev_of(want)
    with _Cap(eng, dec_cap):
        back32, dec = launched(eng, lambda: eng.decompress(dev, output_float=True).cpu().numpy())
        back64 = eng.decompress(dev, output_float=False).cpu().numpy()
    assert same(back32, bank.decoded(want, True)), (name, mode, q, dec_cap, "fp32 decode differs from the oracle's")
    assert same(back64, bank.decoded(want, False)), (name, mode, q, dec_cap, "fp64 decode differs from the oracle's")
    return enc, dec


def quality(bank, name, mode, q):
    """a tolerance is given as a fraction of the field's span"""
    return q * span(bank.field(name)) if mode == 3 else q


# ---- the cap comes and goes -------------------------------------------------------------------------------------
def test_cap_is_restored_when_the_body_fails(eng):
    before = os.environ.get(CAP)
    with pytest.raises(ZeroDivisionError):
        with _Cap(eng, 3):
            assert os.environ[CAP] == "3"
            1 / 0
    assert os.environ.get(CAP) == before
    os.environ[CAP] = "77"
    try:
        with _Cap(eng, 5):
            assert os.environ[CAP] == "5"
        assert os.environ[CAP] == "77"
    finally:
        if before is None:
            os.environ.pop(CAP, None)
        else:
            os.environ[CAP] = before
    assert os.environ.get(CAP) == before


# ---- A: more than 256 chunks of one transformed shape ---------------------------------------------------------------
A1_SETTINGS = [(1, 3.0), (2, 80.0), (3, 1e-3)]


@pytest.mark.parametrize("name", ["a1_f32", "a1_f64"])
@pytest.mark.parametrize("mode,q", A1_SETTINGS)
def test_a1_343_chunks_of_one_shape(eng, bank, name, mode, q):
    """63^3 in 9^3 chunks: batches of 256 and 87 (the fixed-rate encoder: four parts side by side)"""
    assert len(chunk_grid((63, 63, 63), C9)) == 343
    enc, dec = roundtrip(eng, bank, name, C9, mode, quality(bank, name, mode, q))
    enc64, dec64 = roundtrip(eng, bank, "a1_64", C9, mode, quality(bank, "a1_64", mode, q))
    print(name, mode, "encoder", enc[ENC_WITNESS], "against", enc64[ENC_WITNESS], "decoder", dec[DEC_WITNESS], "against",
          dec64[DEC_WITNESS])
    assert dec64[DEC_WITNESS] > 0 and dec[DEC_WITNESS] == 2 * dec64[DEC_WITNESS], (dec[DEC_WITNESS], dec64[DEC_WITNESS])
    if mode != 1:   # (a fixed-rate group of 64 to 512 chunks is cut into four parts: no second batch, see above)
        assert enc64[ENC_WITNESS] > 0 and enc[ENC_WITNESS] == 2 * enc64[ENC_WITNESS], (enc[ENC_WITNESS], enc64[ENC_WITNESS])


def test_a1_729_chunks_at_a_fixed_rate(eng, bank):
    """81^3 in 9^3 chunks: beyond 512 chunks the fixed-rate encoder has no parts either, so its batches are 256, 256
    and 217 -- three times the one batch of 27 chunks; the decoder's three batches have three sub-batches each"""
    assert len(chunk_grid((81, 81, 81), C9)) == 729
    enc, dec = roundtrip(eng, bank, "a1_729", C9, 1, 3.0)
    enc27, _ = roundtrip(eng, bank, "a1_27", C9, 1, 3.0)
    print("a1_729 encoder", enc[ENC_WITNESS], "against", enc27[ENC_WITNESS], "decoder", dec[DEC_WITNESS])
    assert enc27[ENC_WITNESS] == 1 and enc[ENC_WITNESS] == 3 * enc27[ENC_WITNESS], (enc[ENC_WITNESS], enc27[ENC_WITNESS])
    assert dec[DEC_WITNESS] == 9, dec[DEC_WITNESS]


@pytest.mark.parametrize("mode,q", [(1, 2.0), (2, 70.0)])
def test_a2_a_large_group_beside_small_ones(eng, bank, mode, q):
    """(z, y, x) = 66 x 63 x 70 in 9^3 chunks: 294 chunks of 9^3 beside groups of 49, 42 and 7 chunks.  In the decoder
    all four groups are deferred (none takes the table kernels) and the large one is split, 256 + 38.  The encoder
    splits it the same way at a PSNR target; at a fixed rate it cuts the 294 chunks into four parts, which run side
    by side with the small groups (the fallback from side by side is B3's, under the cap)"""
    groups = {}
    for c in chunk_grid((66, 63, 70), C9):
        groups[(c[1], c[3], c[5])] = groups.get((c[1], c[3], c[5]), 0) + 1
    assert sorted(groups.values()) == [7, 42, 49, 294]
    roundtrip(eng, bank, "a2", C9, mode, q)


@pytest.mark.parametrize("mode,q", [(1, 4.0), (3, 1e-3)])
def test_a3_a_group_that_spans_two_volumes(eng, bank, mode, q):
    """two volumes of 150 chunks in one call: one group of 300 chunks, batches of 256 and 44"""
    vols = [bank.field("a3_0"), bank.field("a3_1")]
    assert len(chunk_grid(vols[0].shape, C9)) == 150
    q = quality(bank, "a3_0", mode, q)
    wants = [bank.container(n, C9, mode, q) for n in ("a3_0", "a3_1")]
    assert wants[0] != wants[1]
    parts = eng.compress_batch(cuda(np.stack(vols)), C9, q, mode=mode)
    assert [host(p) for p in parts] == wants
    conts = [dev_of(w) for w in wants]
    for of in (True, False):
        back = eng.decompress_batch(conts, output_float=of).cpu().numpy()
        for v, w in enumerate(wants):
            assert same(back[v], bank.decoded(w, of)), (mode, of, v)


@pytest.mark.parametrize("mode,q", [(1, 2.0), (2, 90.0)])
def test_a4_300_slices(eng, oracle, bank, mode, q):
    """300 slices of 24 x 31 with distinct seeds: batches of 256 and 44 slices, both ways"""
    imgs = bank.get(("slices",), lambda: np.stack([turbulence((1, 24, 31), seed=200 + s)[0] for s in range(300)]))
    wants = [oracle.comp_2d(img, mode, q, False) for img in imgs]
    parts = eng.compress_2d_batch(cuda(imgs), q, mode=mode)
    assert [host(p) for p in parts] == wants
    streams = [dev_of(w) for w in wants]
    for of in (True, False):
        back = eng.decompress_2d_batch(streams, (24, 31), output_float=of).cpu().numpy()
        for s, w in enumerate(wants):
            assert same(back[s], oracle.decomp_2d(w, (24, 31), of)), (mode, of, s)


def test_a5_windows_on_343_chunks(eng, oracle, bank):
    """a box that meets all 343 chunks, cropped on every side, and the first 30 % of every chunk stream"""
    c = bank.container("a1_f32", C9, 1, 3.0)
    dev = dev_of(c)
    lo, dims = (1, 1, 1), (61, 61, 61)
    for of in (True, False):
        assert same(eng.decompress_box(dev, lo, dims, output_float=of), crop(bank.decoded(c, of), lo, dims)), of
        part = bank.get(("t", c, 30), lambda: oracle.trunc_3d(c, 30))
        assert len(part) < len(c)
        assert same(eng.decompress(dev, output_float=of, pct=30), bank.decoded(part, of)), of


# ---- B: the cap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,q", [(1, 2.0), (2, 90.0), (3, 1e-4)])
def test_b1_table_kernel_chunks_one_per_batch(eng, bank, mode, q):
    """64^3 in 32^3 chunks under cap 1: eight batches of one chunk"""
    q = quality(bank, "b1", mode, q)
    enc, dec = roundtrip(eng, bank, "b1", C32, mode, q, enc_cap=1, dec_cap=1)
    if mode == 1:
        enc0, dec0 = roundtrip(eng, bank, "b1", C32, mode, q)
        print("b1 encoder", enc[ENC_WITNESS], "against", enc0[ENC_WITNESS], "decoder", dec[DEC_WITNESS], "against", dec0[DEC_WITNESS])
        assert enc0[ENC_WITNESS] == 1 and enc[ENC_WITNESS] >= 3 * enc0[ENC_WITNESS] and enc[ENC_WITNESS] == 8
        assert dec0[DEC_WITNESS] == 4 and dec[DEC_WITNESS] == 8   # one batch in four sub-batches; eight batches


def wide_planes(container):
    """bit planes of every chunk stream (byte 17 of a chunk, src/SPECK_INT.cpp:284-308)"""
    return [s[17] for s in split_container(container)[3]]


@pytest.mark.parametrize("which,mode,q", [("b2", 1, 2.0), ("b2_wide", 1, 24.0), ("b2_wide", 1, 40.0), ("b2", 3, 1e-4)])
def test_b2_fast_path_chunks_three_per_batch(eng, bank, which, mode, q):
    """128^3 in 64^3 chunks, batches of 3 + 3 + 2: a short last batch, and a middle one below the sub-batch threshold.
    At 40 bpp every chunk takes the 64-bit retry, at 24 bpp chunk 1 of the first and chunk 5 of the second batch (beside
    the ramp, chunk 4) and none of the third; the coder's arrays lie over the chunk buffer, so a batch with a retry
    is transformed again (Engine::wideScratch)"""
    q = quality(bank, which, mode, q)
    if which == "b2_wide":
        planes = wide_planes(bank.container(which, C64, mode, q))
        assert all((p > 32) == (i in WIDE_AT_24 or q == 40.0) for i, p in enumerate(planes)), planes
    redo0 = eng.lib.sperrhip_debug_counter(0)
    enc, dec = roundtrip(eng, bank, which, C64, mode, q, enc_cap=ENC_RATE_64 if mode == 1 else ENC_PWE_64,
                         dec_cap=DEC_RATE_64 if mode == 1 else DEC_PWE_64)
    redo = eng.lib.sperrhip_debug_counter(0) - redo0
    print(which, mode, q, "encoder", enc[ENC_WITNESS], "decoder", dec[DEC_WITNESS], "batches transformed again", redo)
    if which == "b2_wide":   # (at 24 bpp the last batch, chunks 6 and 7, has nothing to retry)
        assert redo == (3 if q == 40.0 else 2), redo
    if (mode, q) == (1, 2.0):
        enc0, dec0 = roundtrip(eng, bank, which, C64, mode, q)
        assert enc0[ENC_WITNESS] == 1 and enc[ENC_WITNESS] >= 3 * enc0[ENC_WITNESS] and enc[ENC_WITNESS] == 3
        assert dec0[DEC_WITNESS] == 4 and dec[DEC_WITNESS] == 3   # one batch in four sub-batches; three batches
    if mode == 3:   # (the tolerance caps rest on measured sizes too: three batches each way)
        assert enc[ENC_WITNESS] == 3 and dec[DEC_WITNESS] == 3


@pytest.mark.parametrize("cap", [1, 4])
@pytest.mark.parametrize("mode,q", [(1, 2.0), (3, 1e-3)])
def test_b3_ragged_volume(eng, bank, cap, mode, q):
    """(z, y, x) = 72 x 80 x 100 in 32^3 chunks: 12 chunks in 8 shape groups, non-dyadic ones among them, deferred in
    the decoder at a fixed rate and decoded in order with a tolerance.  Parity is the only check on drain()"""
    groups = {}
    for c in chunk_grid((72, 80, 100), C32):
        groups[(c[1], c[3], c[5])] = groups.get((c[1], c[3], c[5]), 0) + 1
    assert sorted(groups.values()) == [1, 1, 1, 1, 2, 2, 2, 2]
    q = quality(bank, "b3", mode, q)
    enc, dec = roundtrip(eng, bank, "b3", C32, mode, q, enc_cap=cap, dec_cap=cap)
    if (cap, mode) == (1, 1):
        enc0, dec0 = roundtrip(eng, bank, "b3", C32, mode, q)
        print("b3 encoder", enc[ENC_WITNESS], "against", enc0[ENC_WITNESS], "decoder", dec[DEC_WITNESS], "against", dec0[DEC_WITNESS])
        assert enc0[ENC_WITNESS] == 8 and enc[ENC_WITNESS] == 12   # a batch per group; a batch per chunk
        assert dec0[DEC_WITNESS] == 8 and dec[DEC_WITNESS] == 12


B2_KEY = ("b2", C64, 1, 2.0)
BOX_LO, BOX_DIMS = (5, 9, 3), (101, 97, 111)


def test_b4_box(eng, bank):
    c = bank.container(*B2_KEY)
    dev = dev_of(c)
    assert all(lo < 64 < lo + d <= 128 for lo, d in zip(BOX_LO, BOX_DIMS))   # (meets all 8 chunks)
    with _Cap(eng, DEC_RATE_64):
        got = [eng.decompress_box(dev, BOX_LO, BOX_DIMS, output_float=of).cpu().numpy() for of in (True, False)]
    for of, g in zip((True, False), got):
        assert same(g, crop(bank.decoded(c, of), BOX_LO, BOX_DIMS)), of


def test_b4_levels(eng, bank):
    c = bank.container(*B2_KEY)
    dev = dev_of(c)
    want = bank.levels(c)[1]
    assert len(want) > 1 and len(eng.multires_levels((128, 128, 128), C64)) == len(want)
    with _Cap(eng, DEC_RATE_64):
        got = [eng.decompress_level(dev, h).cpu().numpy() for h in range(len(want))]
    for h, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), h


def test_b4_multires(eng, bank):
    c = bank.container(*B2_KEY)
    dev = dev_of(c)
    want = bank.levels(c)[1]
    with _Cap(eng, DEC_RATE_64):
        got = [eng.decompress_multires(dev, output_float=of) for of in (True, False)]
        got = [(v.cpu().numpy(), [t.cpu().numpy() for t in lv]) for v, lv in got]
    for of, (v, lv) in zip((True, False), got):
        assert same(v, bank.decoded(c, of)), of
        assert len(lv) == len(want) and all(same(g, w) for g, w in zip(lv, want)), of


def test_b4_portion(eng, oracle, bank):
    c = bank.container(*B2_KEY)
    dev = dev_of(c)
    part = oracle.trunc_3d(c, 37)
    assert len(part) < len(c)
    with _Cap(eng, DEC_RATE_64):
        got = [eng.decompress(dev, output_float=of, pct=37).cpu().numpy() for of in (True, False)]
    for of, g in zip((True, False), got):
        assert same(g, oracle.decomp_3d(part, of)), of


B4_THREE = ("b2", "b2_other1", "b2_other2")


def test_b4_batch_of_three_containers(eng, bank):
    wants = [bank.container(n, C64, 1, 2.0) for n in B4_THREE]
    assert len(set(wants)) == 3
    conts = [dev_of(w) for w in wants]
    with _Cap(eng, DEC_RATE_64):
        got = [eng.decompress_batch(conts, output_float=of).cpu().numpy() for of in (True, False)]
    for of, g in zip((True, False), got):
        for v, w in enumerate(wants):
            assert same(g[v], bank.decoded(w, of)), (of, v)


def test_b4_boxes_of_three_entries(eng, bank):
    wants = [bank.container(n, C64, 1, 2.0) for n in B4_THREE]
    conts = [dev_of(w) for w in wants]
    los, dims = [(5, 9, 3), (31, 1, 17), (63, 63, 63)], (65, 65, 64)
    with _Cap(eng, DEC_RATE_64):
        got = [eng.decompress_boxes(conts, los, dims, output_float=of).cpu().numpy() for of in (True, False)]
    for of, g in zip((True, False), got):
        for e, (w, lo) in enumerate(zip(wants, los)):
            assert same(g[e], crop(bank.decoded(w, of), lo, dims)), (of, e)


def test_b4_interleaved_fields(eng, bank):
    vols = [bank.field(n) for n in B4_THREE]
    wants = [bank.container(n, C64, 1, 2.0) for n in B4_THREE]
    t = cuda(np.stack(vols, axis=-1))   # (z, y, x, c), channels last
    with _Cap(eng, ENC_RATE_64):
        parts = [host(p) for p in eng.compress_fields(t, C64, 2.0)]
    assert parts == wants
    conts = [dev_of(w) for w in wants]
    with _Cap(eng, DEC_RATE_64):
        got = [eng.decompress_fields(conts, output_float=of).cpu().numpy() for of in (True, False)]
    for of, g in zip((True, False), got):
        assert g.shape == (128, 128, 128, 3)
        for f, w in enumerate(wants):
            assert same(np.ascontiguousarray(g[..., f]), bank.decoded(w, of)), (of, f)


@pytest.mark.parametrize("mode,q", [(1, 2.0), (2, 90.0), (3, 1e-4)])
def test_b5_a_cap_below_one_chunk(eng, bank, mode, q):
    """one 64^3 chunk needs 5 to 14 MiB: under cap 1 it is coded all the same, one chunk is always allowed"""
    enc, dec = roundtrip(eng, bank, "b5", C64, mode, quality(bank, "b5", mode, q), enc_cap=1, dec_cap=1)
    assert enc[ENC_WITNESS] == 1 and dec[DEC_WITNESS] == 1


def test_b6_leaving_the_cap(eng, bank):
    """the engine that coded under the cap codes the same call without it, in one batch again"""
    before = os.environ.get(CAP)
    roundtrip(eng, bank, "b2", C64, 1, 2.0, enc_cap=ENC_RATE_64, dec_cap=DEC_RATE_64)
    assert os.environ.get(CAP) == before
    enc, dec = roundtrip(eng, bank, "b2", C64, 1, 2.0)
    assert enc[ENC_WITNESS] == 1 and dec[DEC_WITNESS] == 4
