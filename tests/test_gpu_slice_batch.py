"""GPU: a batch of same-shape 2D slices in one call (sperrhip_compress_2d_batch_dev, sperrhip_decompress_2d_batch_dev,
SperrHip.compress_2d_batch / decompress_2d_batch).

Stream s of a batch has to be byte for byte what the oracle (sperr_comp_2d) and the single-slice call make of slice s
alone, and slice s of a batch decode bit for bit the oracle's (sperr_decomp_2d) and the single call's decode of
stream s.  Nothing is compared against the batch itself, and no tolerance is involved.  The cases walk the three
modes in both precisions with and without the 10-byte header, a real 999 x 999 field, truncated and mixed streams in
one decode, the 64-bit retry of some slices of a batch, a group that runs as several batches of 256 chunks, the launch
counts, the refusals and the Python conveniences."""
import ctypes as C
import os

import numpy as np
import pytest

from fields import ramp_field
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu
_sz = C.c_size_t
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def dev_bytes(b):
    return cuda(np.frombuffer(b, dtype=np.uint8))


def check_offsets(parts):
    """the views lie back to back in one buffer, from its start: offsets 0 = o_0 < o_1 < ... < o_N"""
    base = parts[0].untyped_storage().data_ptr()
    at = 0
    for p in parts:
        assert p.data_ptr() - base == at and p.numel() > 0
        at += p.numel()
    return at


def five(shape, dtype):
    return [turbulence((1,) + shape, seed=s, dtype=dtype)[0] for s in (1, 2, 3, 4)] + \
        [np.full(shape, 1.25, dtype=dtype)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(37, 50), (96, 121), (9, 200), (256, 256)])
@pytest.mark.parametrize("mode,q", [(1, 0.7), (1, 5.0), (2, 75.0), (2, 160.0), (3, 1e-2), (3, 1e-6)])
def test_modes_and_precisions(eng, oracle, mode, q, shape, dtype):
    """four turbulence slices and a constant one: every stream equals the oracle's and the single call's, with and
    without header; both decodes equal the oracle's, from headerless and from headered streams"""
    imgs = five(shape, dtype)
    src = cuda(np.stack(imgs))
    bodies = None
    for hdr in (False, True):
        parts = eng.compress_2d_batch(src, q, mode=mode, header=hdr)
        assert len(parts) == len(imgs)
        assert check_offsets(parts) == sum(p.numel() for p in parts)
        wants = [oracle.comp_2d(img, mode, q, hdr) for img in imgs]
        for img, p, want in zip(imgs, parts, wants):
            assert host(p) == want
            assert host(eng.compress_2d(cuda(img), q, mode=mode, header=hdr)) == want
        if not hdr:
            bodies = wants
        else:
            assert [w[10:] for w in wants] == bodies
        for of in (True, False):
            back = eng.decompress_2d_batch(parts, shape, output_float=of, header=hdr).cpu().numpy()
            assert back.shape == (len(imgs),) + shape
            for s, body in enumerate(bodies):
                assert np.array_equal(bits(back[s]), bits(oracle.decomp_2d(body, shape, of))), (s, hdr, of)


def test_real_field_999(eng, oracle):
    """tests/golden/img999.f32 and its seven flips / transposes as eight slices, PSNR 90 dB and rate 2.0"""
    shape = (999, 999)
    img = np.fromfile(os.path.join(GOLD, "img999.f32"), dtype=np.float32).reshape(shape)
    imgs = [np.ascontiguousarray(f(g)) for g in (img, img.T) for f in
            (lambda a: a, lambda a: a[::-1], lambda a: a[:, ::-1], lambda a: a[::-1, ::-1])]
    assert len(imgs) == 8 and len({a.tobytes() for a in imgs}) == 8
    src = cuda(np.stack(imgs))
    for mode, q in ((2, 90.0), (1, 2.0)):
        parts = eng.compress_2d_batch(src, q, mode=mode)
        check_offsets(parts)
        wants = [oracle.comp_2d(a, mode, q, False) for a in imgs]
        assert [host(p) for p in parts] == wants
        back = eng.decompress_2d_batch(parts, shape, output_float=True).cpu().numpy()
        for s, w in enumerate(wants):
            assert np.array_equal(bits(back[s]), bits(oracle.decomp_2d(w, shape, True))), (mode, s)


def test_truncated_and_mixed_streams(eng, oracle):
    """oracle-written streams of one shape in different modes and precisions, some cut to len - 700 and to 60 bytes,
    decoded together: each slice equals the oracle's decode of its own stream"""
    shape = (80, 120)
    a32 = turbulence((1,) + shape, seed=50)[0]
    a64 = turbulence((1,) + shape, seed=51, dtype=np.float64)[0]
    full = [oracle.comp_2d(a32, 1, 3.0, False), oracle.comp_2d(a64, 2, 90.0, False),
            oracle.comp_2d(a32, 3, 1e-2, False), oracle.comp_2d(a64, 1, 6.0, False),
            oracle.comp_2d(a64, 3, 1e-5, False), oracle.comp_2d(np.full(shape, -3.5, dtype=np.float32), 1, 2.0, False)]
    streams = [full[0], full[0][:len(full[0]) - 700], full[0][:60], full[1], full[1][:len(full[1]) - 700], full[2],
               full[2][:len(full[2]) - 700], full[3], full[3][:60], full[4], full[5]]
    for of in (True, False):
        back = eng.decompress_2d_batch([dev_bytes(s) for s in streams], shape, output_float=of).cpu().numpy()
        for i, s in enumerate(streams):
            assert np.array_equal(bits(back[i]), bits(oracle.decomp_2d(s, shape, of))), (i, of)
            one = eng.decompress_2d(dev_bytes(s), shape, of).cpu().numpy()
            assert np.array_equal(bits(back[i]), bits(one)), (i, of)


@pytest.mark.parametrize("bpp", [24.0, 40.0])
def test_wide_retry_inside_a_batch(eng, oracle, bpp):
    """a ramp slice among turbulence slices: at 24 bpp only the turbulence slices take the 64-bit retry (53 / 32 / 53
    bit planes), at 40 bpp all three (53 / 53 / 53)"""
    shape = (64, 64)
    imgs = [turbulence((1,) + shape, seed=30)[0], ramp_field((1,) + shape)[0], turbulence((1,) + shape, seed=31)[0]]
    wants = [oracle.comp_2d(a, 1, bpp, False) for a in imgs]
    assert [w[17] for w in wants] == ([53, 32, 53] if bpp == 24.0 else [53, 53, 53])
    parts = eng.compress_2d_batch(cuda(np.stack(imgs)), bpp)
    assert [host(p) for p in parts] == wants
    assert [host(eng.compress_2d(cuda(a), bpp)) for a in imgs] == wants
    back = eng.decompress_2d_batch(parts, shape, output_float=False).cpu().numpy()
    for s, w in enumerate(wants):
        assert np.array_equal(bits(back[s]), bits(oracle.decomp_2d(w, shape, False)))


def test_many_tiny_slices(eng, oracle):
    """600 slices of 20 x 24: one shape group that runs as three batches of at most 256 chunks"""
    shape, n = (20, 24), 600
    imgs = [turbulence((1,) + shape, seed=100 + s)[0] for s in range(n)]
    parts = eng.compress_2d_batch(cuda(np.stack(imgs)), 3.0)
    assert len(parts) == n
    check_offsets(parts)
    back = eng.decompress_2d_batch(parts, shape).cpu().numpy()
    sample = sorted({0, 255, 256, 511, 512, 599} | set(range(7, n, 33)))
    assert len(sample) == 24
    for s in sample:
        want = oracle.comp_2d(imgs[s], 1, 3.0, False)
        assert host(parts[s]) == want, s
        assert host(eng.compress_2d(cuda(imgs[s]), 3.0)) == want, s
        assert np.array_equal(bits(back[s]), bits(oracle.decomp_2d(want, shape, True))), s
        assert np.array_equal(bits(back[s]), bits(eng.decompress_2d(dev_bytes(want), shape, True).cpu().numpy())), s


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
    """32 copies of one 96 x 121 slice at rate 2.0.  The kernels of a shape group take all its chunks in one launch
    (grid.y), so the batch launches what one single call does plus the layout kernel (the decoder cuts a batch into at
    most four sub-batches), and the loop 32 times that: under an eighth, and the test asks for under a quarter, each
    direction."""
    shape = (96, 121)
    img = turbulence((1,) + shape, seed=80)[0]
    one = cuda(img)
    imgs = cuda(np.stack([img] * 32))
    single = eng.compress_2d(one, 2.0)
    loop_c = _launches(eng, lambda: [eng.compress_2d(one, 2.0) for _ in range(32)])
    batch_c = _launches(eng, lambda: eng.compress_2d_batch(imgs, 2.0))
    print("launches, compression: batch", batch_c, "loop", loop_c)
    assert 0 < batch_c < loop_c / 4, (batch_c, loop_c)
    parts = eng.compress_2d_batch(imgs, 2.0)
    assert all(host(p) == host(single) for p in parts)
    loop_d = _launches(eng, lambda: [eng.decompress_2d(single, shape) for _ in range(32)])
    batch_d = _launches(eng, lambda: eng.decompress_2d_batch(parts, shape))
    print("launches, decompression: batch", batch_d, "loop", loop_d)
    assert 0 < batch_d < loop_d / 4, (batch_d, loop_d)


def test_refusals(eng, oracle):
    """-1, and the output untouched, for every refusal found before decoding starts; compression never writes past
    dst_cap; 2 for a bad mode / quality"""
    import torch
    shape = (20, 24)
    dy, dx = shape
    imgs = [turbulence((1,) + shape, seed=70 + s)[0] for s in range(3)]
    src = cuda(np.stack(imgs))
    wants = [oracle.comp_2d(a, 1, 4.0, False) for a in imgs]
    hwants = [oracle.comp_2d(a, 1, 4.0, True) for a in imgs]
    buf = dev_bytes(b"".join(wants))
    hbuf = dev_bytes(b"".join(hwants))
    offs, hoffs = [0], [0]
    for w, h in zip(wants, hwants):
        offs.append(offs[-1] + len(w))
        hoffs.append(hoffs[-1] + len(h))
    out = torch.full((3,) + shape, 7.5, dtype=torch.float32, device="cuda")
    sentinel = out.clone()

    def dec(srcbuf, o, n, hdr, dims=(dx, dy), cap=None, dst=out, offsets=True):
        arr = (_sz * len(o))(*o) if offsets else None
        return eng.lib.sperrhip_decompress_2d_batch_dev(srcbuf.data_ptr() if srcbuf is not None else None, arr, n, hdr,
                                                        1, *dims, dst.data_ptr() if dst is not None else None,
                                                        out.numel() * 4 if cap is None else cap, eng._stream())

    other = hbuf.clone()   # the second stream's header names 25 x 20
    other[hoffs[1] + 2] = 25
    cases = [
        dict(srcbuf=buf, o=offs, n=0, hdr=0),                                         # no slices
        dict(srcbuf=None, o=offs, n=3, hdr=0),                                        # NULL pointers
        dict(srcbuf=buf, o=offs, n=3, hdr=0, offsets=False),
        dict(srcbuf=buf, o=offs, n=3, hdr=0, dst=None),
        dict(srcbuf=buf, o=offs, n=3, hdr=0, dims=(0, dy)),                           # a zero dim
        dict(srcbuf=buf, o=offs, n=3, hdr=0, dims=(dx, 0)),
        dict(srcbuf=buf, o=offs, n=3, hdr=0, cap=out.numel() * 4 - 4),                # output too small
        dict(srcbuf=buf, o=[0, offs[2], offs[1], offs[3]], n=3, hdr=0),               # decreasing offsets
        dict(srcbuf=buf, o=[0, offs[1], offs[1] + 10, offs[3]], n=3, hdr=0),          # a stream of 10 bytes
        dict(srcbuf=hbuf, o=[0, hoffs[1], hoffs[1] + 20, hoffs[3]], n=3, hdr=1),      # ... behind its header
        dict(srcbuf=other, o=hoffs, n=3, hdr=1),                                      # a header naming other dims
        dict(srcbuf=hbuf, o=hoffs, n=3, hdr=1, dims=(dy, dx)),                        # every header names other dims
    ]
    for kw in cases:
        assert dec(**kw) == -1, kw
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), kw
    assert dec(hbuf, hoffs, 3, 1) == 0   # (the same buffers decode when nothing is wrong)
    torch.cuda.synchronize()
    for s, w in enumerate(wants):
        assert np.array_equal(bits(out[s].cpu().numpy()), bits(oracle.decomp_2d(w, shape, True)))

    # compression
    cap = eng.max_compressed_size_2d_batch(3, shape, 4.0)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    o = (_sz * 4)()

    def comp(n, dims, mode, q, room, hdr=0, d=dst, offsets=o, s=src):
        return eng.lib.sperrhip_compress_2d_batch_dev(s.data_ptr() if s is not None else None, 1, n, *dims, mode, q, hdr,
                                                      d.data_ptr() if d is not None else None, room, offsets,
                                                      eng._stream())

    xy = (dx, dy)
    assert comp(3, xy, 4, 4.0, cap) == 2
    assert comp(3, xy, 0, 4.0, cap) == 2
    assert comp(3, xy, 1, 0.0, cap) == 2
    assert comp(3, xy, 1, -1.0, cap) == 2
    assert comp(0, xy, 1, 4.0, cap) == -1
    assert comp(3, (dx, 0), 1, 4.0, cap) == -1
    assert comp(3, (0, dy), 1, 4.0, cap) == -1
    assert comp(3, xy, 1, 4.0, cap, offsets=None) == -1
    assert comp(3, xy, 1, 4.0, cap, d=None) == -1
    assert comp(3, xy, 1, 4.0, cap, s=None) == -1
    assert comp(2 ** 32, xy, 1, 4.0, cap) == -1   # nslice beyond 2^32 - 1
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    for hdr, ws in ((0, wants), (1, hwants)):   # one byte short: refused, nothing written past the room given
        total = sum(len(w) for w in ws)
        dst.fill_(0xA5)
        assert comp(3, xy, 1, 4.0, total - 1, hdr=hdr) == -1
        torch.cuda.synchronize()
        assert bool((dst[total - 1:] == 0xA5).all())
        assert comp(3, xy, 1, 4.0, total, hdr=hdr) == 0 and o[0] == 0 and o[3] == total
        torch.cuda.synchronize()
        assert host(dst[:total]) == b"".join(ws)
        assert bool((dst[total:] == 0xA5).all())


def test_python_inputs(eng, oracle):
    """separately allocated stream tensors (concatenated by the wrapper), `out=` reuse, a non-default torch stream,
    and a batch of one equal to the single calls"""
    import torch
    shape = (28, 40)
    imgs = [turbulence((1,) + shape, seed=90 + s, dtype=np.float64)[0] for s in range(4)]
    wants = [oracle.comp_2d(a, 1, 3.0, False) for a in imgs]
    conts = [dev_bytes(w) for w in wants]
    src = cuda(np.stack(imgs))
    room = torch.empty(eng.max_compressed_size_2d_batch(4, shape, 3.0) + 64, dtype=torch.uint8, device="cuda")
    vals = torch.empty((4,) + shape, dtype=torch.float64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        parts = eng.compress_2d_batch(src, 3.0, out=room)
        back = eng.decompress_2d_batch(conts, shape, output_float=False)
        again = eng.decompress_2d_batch(parts, shape, output_float=False, out=vals)
    st.synchronize()
    assert parts[0].data_ptr() == room.data_ptr() and again.data_ptr() == vals.data_ptr()
    assert [host(p) for p in parts] == wants
    for s, w in enumerate(wants):
        want = bits(oracle.decomp_2d(w, shape, False))
        assert np.array_equal(bits(back[s].cpu().numpy()), want)
        assert np.array_equal(bits(again[s].cpu().numpy()), want)
    for mode, q, hdr in ((1, 3.0, False), (3, 1e-4, True), (2, 100.0, False)):
        (p,) = eng.compress_2d_batch(src[2:3], q, mode=mode, header=hdr)
        single = eng.compress_2d(src[2], q, mode=mode, header=hdr)
        assert host(p) == host(single) == oracle.comp_2d(imgs[2], mode, q, hdr)
        body = single[10:] if hdr else single
        one = eng.decompress_2d_batch([p], shape, output_float=False, header=hdr).cpu().numpy()
        assert one.shape == (1,) + shape
        assert np.array_equal(bits(one[0]), bits(eng.decompress_2d(body, shape, False).cpu().numpy()))
        assert np.array_equal(bits(one[0]), bits(oracle.decomp_2d(host(body), shape, False)))
