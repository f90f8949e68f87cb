"""GPU: the decoder's tile sweep from a plane's refinement to the next plane's census (k_pix_turn) and the launch that
ends a plane and scans the next (k_dec_turn), speck_dec.hip, against the four kernels they stand for (k_ref_deposit,
k_dec_plane_end, k_dec_count, k_dec_scan).  SPERR_HIP_PIX_TURN: 0 never, 2 wherever the refinement goes through bit
planes, unset the rule of plan_pix_turn (engine.hip: chunks of at least 64 decoder tiles).  A plan reads the switch when
it is made, so every case drops the plans (release) around itself.

  streams that end everywhere around a refinement pass   coder level, against oracle.speck3d_decode
  chunks of one batch with different plane counts          a container of three chunks, against oracle.decomp_3d
  the same bits either way                                 golden 3D containers and two slices, switch 0 against 2
  launches                                                 which kernels run, switch 2, unset above and below the rule

Where the sweep does not apply.  Seen in the launches with the switch at 2 (test_same_bits_either_way asserts it): a
3D chunk with more than 32 bit planes decodes in the 64-bit pass, which has no bit-plane storage and keeps
k_ref_apply2 with the four kernels; slices decode with 32-bit coefficients through the bit planes like 3D chunks and
take the sweep."""
import json
import os

import numpy as np
import pytest

from fields import smooth_field
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu
SWITCH = "SPERR_HIP_PIX_TURN"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ("k_pix_turn", "k_dec_turn")
OLD = ("k_dec_count", "k_ref_deposit", "k_dec_scan", "k_dec_plane_end")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    before = os.environ.get(SWITCH)
    yield e
    if before is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = before
    e.release()


def switch(eng, value):
    """set (or, None, unset) the switch and drop the plans: the next call makes them again and reads it"""
    if value is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = value
    eng.release()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_of(container):
    return cuda(np.frombuffer(container, dtype=np.uint8))


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


def chunk_streams(oracle, container):
    """the chunks' streams (a container of one chunk has the short header, without chunk dims; the reference's chunking
    folds a short remainder into the chunk before it, so the oracle says how many chunks there are)"""
    multi = bool(container[1] & 0x10)
    pos = 20 if multi else 14
    vol = [int(d) for d in np.frombuffer(container, dtype=np.uint32, count=3, offset=2)]
    ch = [int(d) for d in np.frombuffer(container, dtype=np.uint16, count=3, offset=14)] if multi else vol
    nch = len(oracle.chunk_volume(vol, ch))
    lens = np.frombuffer(container, dtype=np.uint32, count=nch, offset=pos)
    offs = pos + 4 * nch + np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]])
    assert int(offs[-1]) + int(lens[-1]) == len(container)
    return [container[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]


def plane_counts(oracle, container):
    """bit planes of every chunk that is not constant (byte 17 of its stream: the coder's header)"""
    return [s[17] for s in chunk_streams(oracle, container) if len(s) >= 26 and not (s[0] & 1)]


# ---- 1. streams that end everywhere around a refinement pass ---------------------------------------------------------

def quantized(oracle, shape, scale, seed):
    """coefficients as test_gpu_parity.quantized makes them"""
    v = oracle.dwt3d(turbulence(shape, seed=seed).astype(np.float64))
    coef, sign, _ = oracle.quantize(v, np.abs(v).max() / scale)
    return coef, sign


def total_bits(stream):
    return int(np.frombuffer(stream, dtype=np.uint64, count=1, offset=1)[0])


def refinement_ends(oracle, coef, sign, nbp):
    """E[p], p = 0 .. nbp - 1: the bit at which plane p's refinement pass ends in the full-depth stream of `coef`.  The
    stream of coef >> p is a prefix of it that stops exactly there, so E[p] is that stream's useful-bit count
    (E[nbp] = 0: nothing before the first plane)."""
    ends = [total_bits(oracle.speck3d_encode(coef >> np.uint64(p), sign, 0)) for p in range(nbp)]
    return ends + [0]


def cuts_around(ends, nbytes):
    """byte lengths of the truncated streams, every plane: the refinement pass cut short (the refMask path), the pass
    whole (to the bit where E[p] is a multiple of 8: nRef == avail - pos, the boundary of the chunk's end), a byte more,
    and the middle of the plane"""
    cuts = set()
    for p in range(len(ends) - 1):
        e = ends[p]
        up = 9 + (e + 7) // 8
        cuts.update((9 + e // 8 - 1, up, up + 1, 9 + ((ends[p + 1] + e) // 2) // 8))
    return sorted(c for c in cuts if 9 <= c <= nbytes)


@pytest.mark.parametrize("shape,seed", [((64, 64, 64), 7), ((41, 64, 64), 42), ((17, 17, 17), 42)])
def test_streams_that_end_around_a_refinement_pass(eng, oracle, shape, seed):
    """16 tiles through the table kernels and tileBorn; 11 tiles, the last partial, mixed-shape lists; one partial tile
    of 77 mask words"""
    coef, sign = quantized(oracle, shape, 3000.0, seed)
    stream = oracle.speck3d_encode(coef, sign, 0)
    nbp = stream[0]
    assert 0 < nbp <= 32
    ends = refinement_ends(oracle, coef, sign, nbp)
    assert ends[0] == total_bits(stream) and all(ends[p] > ends[p + 1] for p in range(nbp))
    aligned = [p for p in range(nbp) if ends[p] % 8 == 0]
    print(shape, "E_p:", ends[:-1], "byte-aligned at planes", aligned)
    assert aligned, "no plane's refinement pass ends on a byte: the boundary nRef == avail - pos is not reached"
    cuts = cuts_around(ends, len(stream))
    switch(eng, "2")
    try:
        _, rep = launched(eng, lambda: eng.speck3d_decode(stream, shape))
        assert rep.get("k_pix_turn", 0) > 0 and not any(k in rep for k in OLD), rep
        for cut in cuts:
            c0, s0 = oracle.speck3d_decode(stream[:cut], shape)
            c1, s1 = eng.speck3d_decode(stream[:cut], shape)
            assert np.array_equal(c0, c1), (shape, cut, "coefficients")
            assert np.array_equal(s0, s1), (shape, cut, "signs")
    finally:
        switch(eng, None)


# ---- 2. chunks of one batch with different plane counts --------------------------------------------------------------

@pytest.mark.parametrize("label,mode,quality,differ", [("psnr", 2, 80.0, False), ("pwe", 3, 1e-3, True)])
def test_chunks_of_one_batch_with_different_plane_counts(eng, oracle, label, mode, quality, differ):
    """Three 64^3 chunks in one batch: as generated, scaled by 1/64, constant.  The launcher runs the planes of the
    deepest chunk, so a shallower one sits out the first turns (p >= nbp) and starts in a census-only one.
    At a PSNR target the quantisation step follows each chunk's own range (the chunk headers: q = 1.73e-3 and 3.40e-5),
    so the scaled chunk has the 15 bit planes of the other and the case only decodes a batch with a constant chunk in
    it.  At a point-wise error tolerance the step is the same for every chunk (1.5 * tolerance) and the plane counts
    are 15 and 10: that container is the one that reaches p >= nbp, and the test asserts it from the headers."""
    v = turbulence((192, 64, 64))
    v[64:128] *= np.float32(1.0 / 64.0)
    v[128:] = 0.5
    c = oracle.comp_3d(v, (64, 64, 64), mode, quality)
    nbps = plane_counts(oracle, c)
    print(label, "bit planes of the chunks:", nbps)
    assert len(nbps) == 2 and 0 < min(nbps) and max(nbps) <= 32
    if differ:
        assert nbps[0] != nbps[1]
    ref = oracle.decomp_3d(c, True)
    switch(eng, "2")
    try:
        back, rep = launched(eng, lambda: eng.decompress(dev_of(c), output_float=True).cpu().numpy())
        assert rep.get("k_pix_turn", 0) > 0 and not any(k in rep for k in OLD), rep
        assert back.shape == ref.shape and np.array_equal(back.view(np.uint32), ref.view(np.uint32))
    finally:
        switch(eng, None)


# ---- 3. the same bits either way ---------------------------------------------------------------------------------------

with open(os.path.join(GOLD, "golden.json")) as f:
    CASES = json.load(f)["cases"]


def decode_both(eng, fn):
    """fn() decoded with the switch at 0 and at 2: the two results and the launches of each"""
    try:
        switch(eng, "0")
        a, ra = launched(eng, fn)
        switch(eng, "2")
        b, rb = launched(eng, fn)
    finally:
        switch(eng, None)
    assert not any(k in ra for k in NEW), ra
    return a, b, ra, rb


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_same_bits_either_way(eng, oracle, case):
    """every 3D container of the golden set.  Chunks of at most 32 bit planes take the sweep; the 64-bit pass of the
    others has no bit planes to deposit into and keeps k_ref_apply2 and the four kernels -- both read off the launches"""
    with open(os.path.join(GOLD, case["tag"] + ".sperr"), "rb") as f:
        c = f.read()
    nbps = plane_counts(oracle, c)
    narrow, wide = any(0 < n <= 32 for n in nbps), any(n > 32 for n in nbps)
    dev = dev_of(c)
    for of in (True, False):
        a, b, ra, rb = decode_both(eng, lambda: eng.decompress(dev, of).cpu().numpy())
        print(case["tag"], "float" if of else "double", "planes", nbps,
              "sweep" if "k_pix_turn" in rb else "-", "no bit planes" if "k_ref_apply2<uint64_t>" in rb else "-")
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), case["tag"]
        assert ("k_pix_turn" in rb) == narrow and rb.get("k_pix_turn", 0) == rb.get("k_dec_turn", 0), rb
        assert ("k_ref_apply2<uint64_t>" in rb) == wide and ("k_dec_count" in rb) == wide, rb
        assert "k_ref_deposit" not in rb, rb
        gone = {k: n for k, n in ra.items() if k not in OLD}
        kept = {k: n for k, n in rb.items() if k not in OLD + NEW}
        assert gone == kept, (gone, kept)


@pytest.mark.parametrize("shape", [(37, 50), (96, 121)])
def test_same_bits_either_way_slices(eng, shape):
    """slices at 2 bits per sample: 32-bit coefficients through the bit planes, so they take the sweep with the switch
    at 2 (a slice is far below the rule's 64 tiles)"""
    img = np.ascontiguousarray(turbulence((3,) + shape)[1])
    switch(eng, None)
    s = eng.compress_2d(cuda(img), 2.0, mode=1)
    for of in (True, False):
        a, b, ra, rb = decode_both(eng, lambda: eng.decompress_2d(s, shape, of).cpu().numpy())
        print(shape, "float" if of else "double", {k: rb.get(k, 0) for k in NEW + OLD + ("k_ref_apply2<uint32_t>",)})
        assert a.tobytes() == b.tobytes()
        assert rb.get("k_pix_turn", 0) > 0 and rb["k_pix_turn"] == rb.get("k_dec_turn", 0), rb
        assert not any(k in rb for k in OLD) and not any("k_ref_apply2" in k for k in rb), rb


# ---- 4. launches ---------------------------------------------------------------------------------------------------------

def test_launches_with_the_switch_on(eng, oracle):
    """64^3 in 32^3 chunks at 2 bits per sample: two launches where there were four, in equal numbers, nothing else moves"""
    v = turbulence((64, 64, 64))
    c = oracle.comp_3d(v, (32, 32, 32), 1, 2.0)
    dev = dev_of(c)
    a, b, ra, rb = decode_both(eng, lambda: eng.decompress(dev, True).cpu().numpy())
    print("switch 0:", ra)
    print("switch 2:", rb)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(b.view(np.uint32), oracle.decomp_3d(c, True).view(np.uint32))
    assert all(ra.get(k, 0) > 0 for k in OLD), ra
    assert rb.get("k_pix_turn", 0) > 0 and rb["k_pix_turn"] == rb.get("k_dec_turn", 0), rb
    assert not any(k in rb for k in OLD), rb
    assert {k: n for k, n in ra.items() if k not in OLD} == {k: n for k, n in rb.items() if k not in NEW}


def test_the_rule_takes_a_chunk_of_64_tiles(eng, oracle):
    """switch unset: one chunk of 128 x 128 x 64 is 64 decoder tiles, the rule's floor"""
    v = turbulence((64, 128, 128))
    c = oracle.comp_3d(v, (128, 128, 64), 1, 2.0)
    switch(eng, None)
    back, rep = launched(eng, lambda: eng.decompress(dev_of(c), True).cpu().numpy())
    print(rep)
    assert rep.get("k_pix_turn", 0) > 0 and rep["k_pix_turn"] == rep.get("k_dec_turn", 0), rep
    assert not any(k in rep for k in OLD), rep
    assert np.array_equal(back.view(np.uint32), oracle.decomp_3d(c, True).view(np.uint32))


def test_the_rule_leaves_a_chunk_of_16_tiles(eng, oracle):
    """switch unset: one chunk of 64^3 keeps the four kernels"""
    v = turbulence((64, 64, 64))
    c = oracle.comp_3d(v, (64, 64, 64), 1, 2.0)
    switch(eng, None)
    back, rep = launched(eng, lambda: eng.decompress(dev_of(c), True).cpu().numpy())
    print(rep)
    assert all(rep.get(k, 0) > 0 for k in OLD) and not any(k in rep for k in NEW), rep
    assert np.array_equal(back.view(np.uint32), oracle.decomp_3d(c, True).view(np.uint32))
