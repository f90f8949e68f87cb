"""GPU: a batch of same-shape volumes in one call (sperrhip_compress_batch_dev, sperrhip_decompress_batch_dev,
SperrHip.compress_batch / decompress_batch).

Container v of a batch has to be byte for byte what the oracle (and the single-volume call) makes of volume v
alone, and volume v of a batch decode bit for bit the oracle's (and the single call's) decode of container v.
The cases walk the three modes in both precisions, single-chunk containers, dyadic chunks (the table list
kernels), the 64-bit retry of some chunks of a batch, many tiny volumes, containers of different chunk dims,
modes and truncation in one decode, the refusals and the launch counts."""
import ctypes as C

import numpy as np
import pytest

from fields import ramp_field
from sperr_amd import api
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu
_sz = C.c_size_t


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    return SperrHip()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def host(t):
    return bytes(t.cpu().numpy())


def stack(vols):
    return cuda(np.stack(vols))


def check_offsets(parts):
    """the views lie back to back in one buffer, from its start: offsets 0 = o_0 < o_1 < ... < o_N"""
    base = parts[0].untyped_storage().data_ptr()
    at = 0
    for p in parts:
        assert p.data_ptr() - base == at and p.numel() > 0
        at += p.numel()
    return at


def five(shape, dtype):
    return [turbulence(shape, seed=s, dtype=dtype) for s in (1, 2, 3, 4)] + [np.full(shape, 1.25, dtype=dtype)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode,q", [(1, 2.0), (2, 80.0), (3, 1e-3)])
def test_modes_and_precisions(eng, oracle, mode, q, dtype):
    """four turbulence volumes and a constant one, 32^3 chunks of 40 x 48 x 56: several shape groups, merged
    remainders; every container equals the oracle's and the single call's"""
    vols = five((40, 48, 56), dtype)
    parts = eng.compress_batch(stack(vols), (32, 32, 32), q, mode=mode)
    assert len(parts) == len(vols)
    total = check_offsets(parts)
    assert total == sum(p.numel() for p in parts)
    for v, p in zip(vols, parts):
        want = oracle.comp_3d(v, (32, 32, 32), mode, q)
        assert host(p) == want
        assert host(eng.compress(cuda(v), (32, 32, 32), q, mode=mode)) == want
    back = eng.decompress_batch(parts, output_float=True).cpu().numpy()
    for v, p in enumerate(parts):
        assert np.array_equal(bits(back[v]), bits(oracle.decomp_3d(host(p), True)))


def test_single_chunk_containers(eng, oracle):
    """chunk dims at least the volume's: one chunk per container, 14-byte headers"""
    vols = [turbulence((16, 20, 24), seed=10 + s) for s in range(7)]
    for ch in ((24, 20, 16), (64, 64, 64)):
        parts = eng.compress_batch(stack(vols), ch, 3.0)
        check_offsets(parts)
        for v, p in zip(vols, parts):
            want = oracle.comp_3d(v, ch, 1, 3.0)
            assert want[1] & 0x10 == 0 and host(p) == want
        back = eng.decompress_batch(parts, output_float=False).cpu().numpy()
        for v, p in enumerate(parts):
            assert np.array_equal(bits(back[v]), bits(oracle.decomp_3d(host(p), False)))


@pytest.mark.parametrize("bpp", [2.0, 8.0])
def test_dyadic_batch(eng, oracle, bpp):
    """four 64^3 volumes in 32^3 chunks: 32 chunks of one dyadic shape, the table list kernels"""
    vols = [turbulence((64, 64, 64), seed=20 + s) for s in range(4)]
    parts = eng.compress_batch(stack(vols), (32, 32, 32), bpp)
    wants = [oracle.comp_3d(v, (32, 32, 32), 1, bpp) for v in vols]
    assert [host(p) for p in parts] == wants
    for of in (True, False):
        back = eng.decompress_batch(parts, output_float=of).cpu().numpy()
        for v, w in enumerate(wants):
            assert np.array_equal(bits(back[v]), bits(oracle.decomp_3d(w, of)))


@pytest.mark.parametrize("bpp", [24.0, 40.0])
def test_wide_retry_of_some_chunks(eng, oracle, bpp):
    """a ramp volume among turbulence volumes: at 24 bpp only the turbulence chunks take the 64-bit retry (the ramp's
    32 planes fill the budget), at 40 bpp all of them; with 64^3 chunks the coder arrays lie over the chunk buffer
    and the retry transforms the batch again"""
    eng.lib.sperrhip_debug_counter.restype = C.c_ulonglong
    eng.lib.sperrhip_debug_counter.argtypes = [C.c_int]
    for shape, ch in (((32, 32, 32), (32, 32, 32)), ((64, 64, 64), (64, 64, 64))):
        vols = [turbulence(shape, seed=30), ramp_field(shape), turbulence(shape, seed=31)]
        redo0 = eng.lib.sperrhip_debug_counter(0)
        parts = eng.compress_batch(stack(vols), ch, bpp)
        wants = [oracle.comp_3d(v, ch, 1, bpp) for v in vols]
        planes = [w[18 + 17] for w in wants]
        assert planes[0] > 32 and planes[2] > 32 and (planes[1] > 32) == (bpp == 40.0), planes
        assert [host(p) for p in parts] == wants
        if shape[0] == 64:
            assert eng.lib.sperrhip_debug_counter(0) > redo0, "the retry did not transform the batch again"
        back = eng.decompress_batch(parts, output_float=False).cpu().numpy()
        for v, w in enumerate(wants):
            assert np.array_equal(bits(back[v]), bits(oracle.decomp_3d(w, False)))


def test_many_tiny_volumes(eng, oracle):
    """300 volumes of 12 x 10 x 9: one shape group of 300 chunks"""
    vols = [turbulence((9, 10, 12), seed=100 + s) for s in range(300)]
    parts = eng.compress_batch(stack(vols), (32, 32, 32), 4.0)
    check_offsets(parts)
    singles = [eng.compress(cuda(v), (32, 32, 32), 4.0) for v in vols]
    assert [host(p) for p in parts] == [host(s) for s in singles]
    for v in range(0, 300, 30):
        assert host(parts[v]) == oracle.comp_3d(vols[v], (32, 32, 32), 1, 4.0)
    back = eng.decompress_batch(parts).cpu().numpy()
    for v, s in enumerate(singles):
        assert np.array_equal(bits(back[v]), bits(eng.decompress(s).cpu().numpy()))


def test_mixed_containers(eng, oracle):
    """oracle-written containers of one volume shape that differ in chunk dims, mode, rate and precision, one of
    them truncated to 30 %, decoded together"""
    shape = (40, 48, 56)
    v32, v64 = turbulence(shape, seed=50), turbulence(shape, seed=51, dtype=np.float64)
    streams = [oracle.comp_3d(v32, (32, 32, 32), 1, 2.0),
               oracle.comp_3d(v64, (24, 20, 16), 2, 90.0),
               oracle.comp_3d(v32, (64, 64, 64), 3, 1e-2),
               oracle.trunc_3d(oracle.comp_3d(v64, (16, 16, 16), 1, 6.0), 30),
               oracle.comp_3d(v32, (32, 32, 32), 1, 0.5)]
    conts = [cuda(np.frombuffer(s, dtype=np.uint8)) for s in streams]
    for of in (True, False):
        back = eng.decompress_batch(conts, output_float=of).cpu().numpy()
        assert back.shape == (len(streams),) + shape
        for v, s in enumerate(streams):
            assert np.array_equal(bits(back[v]), bits(oracle.decomp_3d(s, of)))


def test_batch_of_one(eng, oracle):
    v = turbulence((40, 48, 56), seed=60)
    for mode, q in ((1, 2.0), (3, 1e-3)):
        (p,) = eng.compress_batch(stack([v]), (32, 32, 32), q, mode=mode)
        single = eng.compress(cuda(v), (32, 32, 32), q, mode=mode)
        assert host(p) == host(single) == oracle.comp_3d(v, (32, 32, 32), mode, q)
        back = eng.decompress_batch([p]).cpu().numpy()
        assert np.array_equal(bits(back[0]), bits(eng.decompress(single).cpu().numpy()))


def _dec(eng, src, offs, nvol, out, cap=None):
    o = (_sz * len(offs))(*offs)
    return eng.lib.sperrhip_decompress_batch_dev(src.data_ptr(), o, nvol, 1, out.data_ptr(),
                                                 out.numel() * 4 if cap is None else cap, None, None, None,
                                                 eng._stream())


def test_refusals(eng):
    """-1, and the output untouched, for every refusal found before decoding starts; 2 for a bad mode/quality"""
    import torch
    shape = (16, 20, 24)
    vols = [turbulence(shape, seed=70 + s) for s in range(3)]
    parts = eng.compress_batch(stack(vols), (16, 16, 16), 2.0)
    buf = torch.cat(parts)
    offs = [0]
    for p in parts:
        offs.append(offs[-1] + p.numel())
    out = torch.full((3,) + shape, 7.5, dtype=torch.float32, device="cuda")
    sentinel = out.clone()
    other = eng.compress(cuda(turbulence((16, 20, 25))), (16, 16, 16), 2.0)   # other volume dims
    mixed = torch.cat([parts[0], other])
    bad = buf.clone()
    bad[offs[1]] ^= 0xff   # the second container's version byte
    flip = buf.clone()
    flip[offs[2] + 2] ^= 0x01   # the third container's x dim
    cases = [
        (buf, [0, offs[2], offs[1], offs[3]], 3, None),               # decreasing offsets
        (buf, offs, 0, None),                                          # nvol 0
        (buf, offs, 3, out.numel() * 4 - 4),                           # output too small
        (mixed, [0, parts[0].numel(), mixed.numel()], 2, None),        # volume dims disagree
        (bad, offs, 3, None),                                          # damaged header
        (flip, offs, 3, None),                                         # one x dim changed: other dims, chunk count
        (buf, [0, offs[1], offs[2], offs[3] - 1], 3, None),            # a container cut short
    ]
    for src, o, n, cap in cases:
        assert _dec(eng, src, o, n, out, cap) == -1, (o, n, cap)
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel)
    null = eng.lib.sperrhip_decompress_batch_dev(buf.data_ptr(), None, 3, 1, out.data_ptr(), out.numel() * 4,
                                                 None, None, None, eng._stream())
    assert null == -1 and torch.equal(out, sentinel)
    # compression
    src = stack(vols)
    dst = torch.full((eng.max_compressed_size_batch(3, shape, (16, 16, 16), 2.0),), 0xA5, dtype=torch.uint8,
                     device="cuda")
    o = (_sz * 4)()

    def comp(n, dims, mode, q, cap, d=dst, offsets=o):
        return eng.lib.sperrhip_compress_batch_dev(src.data_ptr(), 1, n, *dims, 16, 16, 16, mode, q, d.data_ptr()
                                                   if d is not None else None, cap, offsets, eng._stream())

    xyz = (24, 20, 16)
    assert comp(3, xyz, 4, 2.0, dst.numel()) == 2
    assert comp(3, xyz, 1, 0.0, dst.numel()) == 2
    assert comp(0, xyz, 1, 2.0, dst.numel()) == -1
    assert comp(3, (24, 0, 16), 1, 2.0, dst.numel()) == -1
    assert comp(3, xyz, 1, 2.0, dst.numel(), offsets=None) == -1
    assert comp(3, xyz, 1, 2.0, dst.numel(), d=None) == -1
    assert comp(2 ** 20, (24, 20, 2 ** 13), 1, 2.0, dst.numel()) == -1   # nvol * dimz > 2^32 - 1
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    # too small: refused, nothing written past the room given
    total = sum(p.numel() for p in parts)
    assert comp(3, xyz, 1, 2.0, total - 1) == -1
    torch.cuda.synchronize()
    assert bool((dst[total - 1:] == 0xA5).all())
    assert comp(3, xyz, 1, 2.0, dst.numel()) == 0 and o[3] == total
    assert host(dst[:total]) == host(buf)


def _launches(eng, fn):
    import torch
    torch.cuda.synchronize()
    eng.profile(True)
    fn()
    torch.cuda.synchronize()
    rep = eng.profile_report()
    eng.profile(False)
    return sum(n for _, n in rep.values())


def test_launch_count(eng):
    """48 copies of a 40 x 48 x 56 volume in 32^3 chunks (two chunk shapes).  A single call codes two shape groups of
    one chunk; the batch codes the same two groups with 48 chunks each.  A group's kernels take all its chunks in
    one launch (grid.y), so a group batch launches what a one-chunk group does, except that the encoder cuts a
    fixed-rate group of 64 to 512 chunks into at most four parts (48: one), and the decoder cuts a batch of a
    shape the table kernels take into at most four sub-batches (these shapes are not dyadic and decode as deferred
    groups: one).  So the batch launches at most 4 x (two groups' launches) + the container kernel, and 48 single
    calls 48 x (two groups' launches): under a twelfth, and the test asks for under a quarter, each direction."""
    v = turbulence((40, 48, 56), seed=80)
    vols = stack([v] * 48)
    one = cuda(v)
    single = eng.compress(one, (32, 32, 32), 2.0)
    loop_c = _launches(eng, lambda: [eng.compress(one, (32, 32, 32), 2.0) for _ in range(48)])
    batch_c = _launches(eng, lambda: eng.compress_batch(vols, (32, 32, 32), 2.0))
    assert 0 < batch_c < loop_c / 4, (batch_c, loop_c)
    parts = eng.compress_batch(vols, (32, 32, 32), 2.0)
    assert all(host(p) == host(single) for p in parts)
    loop_d = _launches(eng, lambda: [eng.decompress(single) for _ in range(48)])
    batch_d = _launches(eng, lambda: eng.decompress_batch(parts))
    assert 0 < batch_d < loop_d / 4, (batch_d, loop_d)


def test_python_inputs(eng, oracle):
    """separately allocated containers (concatenated by decompress_batch) and a non-default torch stream"""
    import torch
    vols = [turbulence((24, 28, 40), seed=90 + s, dtype=np.float64) for s in range(4)]
    streams = [oracle.comp_3d(v, (16, 16, 16), 1, 3.0) for v in vols]
    conts = [cuda(np.frombuffer(s, dtype=np.uint8)) for s in streams]
    s = torch.cuda.Stream()
    src = stack(vols)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        parts = eng.compress_batch(src, (16, 16, 16), 3.0)
        back = eng.decompress_batch(conts, output_float=False)
        again = eng.decompress_batch(parts, output_float=False)
    s.synchronize()
    assert [host(p) for p in parts] == streams
    for v, w in enumerate(streams):
        want = bits(oracle.decomp_3d(w, False))
        assert np.array_equal(bits(back[v].cpu().numpy()), want)
        assert np.array_equal(bits(again[v].cpu().numpy()), want)


def test_exports_are_wired(eng):
    for name in ("sperrhip_max_compressed_size_batch", "sperrhip_compress_batch_dev",
                 "sperrhip_decompress_batch_dev"):
        assert name in api.EXPORTS
