"""GPU: a portion of a 3D container -- truncating on the device (sperrhip_trunc_dev / _batch_dev, k_trunc_container)
and decoding the first pct percent of every chunk stream without making the truncated container
(sperrhip_decompress_portion_dev, sperrhip_decomp_3d_portion).

Containers come from eng.compress on sperr_amd.synth.turbulence fields (one fabricated one aside).  Expected values are
always the oracle's: oracle.trunc_3d for the bytes, oracle.decomp_3d / decomp_3d_multi_res of oracle.trunc_3d(c, pct)
for the values, cut with numpy.  All compares are on the bit patterns.  Every decode case also asserts that the
expectation differs from the oracle's full decode, so a decoder that reads past a kept prefix cannot pass."""
import ctypes as C

import numpy as np
import pytest

from fields import smooth_field
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


def dev_of(container):
    return cuda(np.frombuffer(container, dtype=np.uint8))


def host_of(t):
    return bytes(t.cpu().numpy())


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def crop(full, lo, dims):
    return np.ascontiguousarray(full[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])


def table(container):
    """the chunk lengths of a container"""
    multi = bool(container[1] & 0x10)
    pos = 20 if multi else 14
    n = 1
    if multi:
        vol = np.frombuffer(container, dtype=np.uint32, count=3, offset=2)
        ch = np.frombuffer(container, dtype=np.uint16, count=3, offset=14)
        for v, c in zip(vol, ch):
            v, c = int(v), int(c)
            n *= max(1, v // c + (1 if v % c > c // 2 else 0))
    return [int(x) for x in np.frombuffer(container, dtype=np.uint32, count=n, offset=pos)]


def _fields():
    def fixed():
        return turbulence((64, 64, 64))

    def mixed():
        v = turbulence((32, 32, 64))
        v[:, :, :32] = 1.25
        return v

    def tiny():
        return (np.arange(4 * 6 * 9, dtype=np.float64).reshape((4, 6, 9)) * 0.37 + 0.1) ** 2

    def wide():
        v = smooth_field((32, 32, 64), dtype=np.float64)
        v[:, :, :32] = 0.75
        return v

    # name: (field, chunks xyz, quality, mode)
    return {
        "fixed": (fixed, (32, 32, 32), 4.0, 1),            # 8 chunks of 16 410 bytes
        "fine": (fixed, (16, 16, 16), 4.0, 1),             # 64 chunks of 2 074 bytes
        "mixed": (mixed, (32, 32, 32), 2.0, 1),            # a constant chunk (17 bytes) beside a coded one (8 218)
        "tiny": (tiny, (3, 2, 2), 1e-3, 3),                # 18 chunks of at most 64 bytes, fp64 data
        "single64": (lambda: turbulence((32, 32, 32)).astype(np.float64), (32, 32, 32), 4.0, 1),   # 14-byte header
        "ragged": (lambda: turbulence((70, 40, 300)), (256, 32, 32), 2.0, 1),   # merged remainder, k_lis_mx
        "pwe": (lambda: turbulence((48, 32, 48)), (16, 16, 24), 1e-3, 3),
        "wide": (wide, (32, 32, 32), 230.0, 2),            # more than 32 bit planes
    }


class Bank:
    """containers and the oracle's results for them, each made once"""

    def __init__(self, eng, oracle):
        self.eng, self.oracle, self.fields, self.memo = eng, oracle, _fields(), {}

    def get(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def container(self, name):
        def make():
            f, ch, q, mode = self.fields[name]
            return host_of(self.eng.compress(cuda(f()), ch, q, mode=mode))
        return self.get(("c", name), make)

    def dev(self, name):
        return self.get(("d", name), lambda: dev_of(self.container(name)))

    def trunc(self, name, pct):
        return self.get(("t", name, pct), lambda: self.oracle.trunc_3d(self.container(name), pct))

    def decoded(self, name, pct, of):
        """the oracle's decode of the truncated container (pct None: of the container itself)"""
        src = self.container(name) if pct is None else self.trunc(name, pct)
        return self.get(("v", name, pct, of), lambda: self.oracle.decomp_3d(src, of))

    def levels(self, name, pct):
        return self.get(("l", name, pct), lambda: self.oracle.decomp_3d_multi_res(self.trunc(name, pct))[1])


@pytest.fixture(scope="module")
def bank(eng, oracle):
    return Bank(eng, oracle)


def fabricated(nx=80, ny=80, nz=12, seed=5):
    """nx ny nz chunks of one voxel each with streams of 1 .. 199 random bytes: truncation never looks into a stream"""
    n = nx * ny * nz
    lens = np.random.default_rng(seed).integers(1, 200, size=n, dtype=np.uint32)
    head = bytes([0, 0x40 | 0x20 | 0x10]) + np.array([nx, ny, nz], dtype=np.uint32).tobytes() + \
        np.array([1, 1, 1], dtype=np.uint16).tobytes() + lens.tobytes()
    body = np.random.default_rng(seed + 1).integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    return head + body, n, lens


# ---- 1. truncate is byte-identical to oracle.trunc_3d -------------------------------------------------------------------

def test_containers_are_what_the_cases_assume(bank):
    assert table(bank.container("fixed")) == [16410] * 8
    assert table(bank.container("fine")) == [2074] * 64
    assert table(bank.container("mixed")) == [17, 8218]
    t = table(bank.container("tiny"))
    assert len(t) == 18 and max(t) <= 64
    assert not bank.container("single64")[1] & 0x10 and len(table(bank.container("single64"))) == 1
    assert bank.container("wide")[20 + 8 + 17 + 17] > 32


@pytest.mark.parametrize("name,pct", [("fixed", 1), ("fixed", 10), ("fixed", 37), ("fixed", 50), ("fixed", 99),
                                      ("fine", 1), ("fine", 25), ("mixed", 20), ("mixed", 50), ("tiny", 50),
                                      ("single64", 30), ("ragged", 40), ("pwe", 97), ("wide", 40)])
def test_truncate_is_the_oracles_bytes(eng, bank, name, pct):
    want = bank.trunc(name, pct)
    got = host_of(eng.truncate(bank.dev(name), pct))
    assert got == want
    assert got[1] & 0x80 and len(got) <= len(bank.container(name))
    if name == "fine" and pct == 1:
        assert table(got) == [64] * 64
    if name == "tiny":   # nothing to cut: only the flag changes, and the data stay marked fp64
        assert got[2:] == bank.container(name)[2:] and not got[1] & 0x20


@pytest.mark.parametrize("pct", [0, 100, 150])
def test_truncate_whole_is_the_input(eng, bank, pct):
    c = bank.container("fixed")
    got = host_of(eng.truncate(bank.dev("fixed"), pct))
    assert got == c == bank.trunc("fixed", pct) and not got[1] & 0x80


def test_truncate_twice(eng, bank, oracle):
    once = eng.truncate(bank.dev("fixed"), 50)
    twice = host_of(eng.truncate(once, 50))
    assert twice == oracle.trunc_3d(bank.trunc("fixed", 50), 50)
    assert table(twice) == [4102] * 8


def test_truncate_any_alignment(eng, bank):
    """source and destination at odd addresses, and into a buffer of the caller"""
    import torch
    c = bank.container("fixed")
    want = bank.trunc("fixed", 37)
    for so, do in [(1, 0), (3, 5), (8, 7), (4, 4)]:
        src = torch.zeros(len(c) + 16, dtype=torch.uint8, device="cuda")
        src[so:so + len(c)] = bank.dev("fixed")
        out = torch.full((len(c) + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        got = eng.truncate(src[so:so + len(c)], 37, out=out[do:])
        assert got.data_ptr() == out.data_ptr() + do
        assert host_of(got) == want, (so, do)
        rest = out.cpu().numpy()
        assert (rest[:do] == 0xA5).all() and (rest[do + len(want):] == 0xA5).all(), (so, do)


@pytest.mark.parametrize("pct", [50, 100])
def test_truncate_more_chunks_than_a_grid_extent(eng, oracle, pct):
    """76 800 chunks of 1 .. 199 bytes: more than the 65 535 a grid's y extent takes"""
    c, n, lens = fabricated()
    assert n == 76800 > 65535
    want = oracle.trunc_3d(c, pct)
    got = host_of(eng.truncate(dev_of(c), pct))
    assert got == want
    if pct == 50:
        kept = np.frombuffer(got, dtype=np.uint32, count=n, offset=20)
        assert (kept[lens <= 64] == lens[lens <= 64]).all() and (kept[(lens > 64) & (lens < 130)] == 64).all()


def test_truncate_batch(eng, bank):
    """a fixed-rate, a point-wise-error and an fp64 single-chunk container in one call: each its own truncation"""
    import torch
    names = ["fixed", "pwe", "single64"]
    for pct in (37, 100):
        got = eng.truncate_batch([bank.dev(n) for n in names], pct)
        assert [host_of(g) for g in got] == [bank.trunc(n, pct) for n in names]
        assert all(b.data_ptr() == a.data_ptr() + a.numel() for a, b in zip(got, got[1:]))
    # containers that already lie back to back are read where they are
    packed = torch.cat([bank.dev(n) for n in names])
    cuts = np.cumsum([0] + [len(bank.container(n)) for n in names])
    views = [packed[cuts[i]:cuts[i + 1]] for i in range(3)]
    assert [host_of(g) for g in eng.truncate_batch(views, 10)] == [bank.trunc(n, 10) for n in names]


# ---- 2. decompress(pct=...) is the oracle's decode of the truncated container ------------------------------------------

def differing(a, b):
    return int((bits(a) != bits(b)).sum())


@pytest.mark.parametrize("name,pct", [("fixed", 10), ("fixed", 37), ("fixed", 99), ("fine", 25), ("pwe", 60), ("pwe", 97),
                                      ("pwe", 99), ("wide", 40), ("ragged", 40), ("mixed", 20)])
def test_portion_decode_is_the_truncated_containers(eng, bank, name, pct):
    for of in (True, False):
        want = bank.decoded(name, pct, of)
        assert differing(want, bank.decoded(name, None, of)) > 0
        got = eng.decompress(bank.dev(name), of, pct=pct).cpu().numpy()
        assert same(got, want), (name, pct, of)
    if (name, pct) == ("pwe", 99):   # every cut lies in an outlier tail: only the correctors go
        assert differing(bank.decoded(name, pct, True), bank.decoded(name, None, True)) == 569


@pytest.mark.parametrize("pct", [100, 150])
def test_portion_decode_of_everything(eng, bank, pct):
    got = eng.decompress(bank.dev("fixed"), True, pct=pct).cpu().numpy()
    assert same(got, bank.decoded("fixed", None, True))


# ---- 3. box x pct, level x pct ------------------------------------------------------------------------------------------

BOXES = [((5, 7, 9), (40, 30, 21)),      # odd origin, across the chunk borders of every axis
         ((63, 31, 32), (1, 1, 1)),      # one voxel
         ((32, 0, 32), (32, 32, 32))]    # one chunk


@pytest.mark.parametrize("lo,dims", BOXES)
def test_box_of_a_portion(eng, bank, lo, dims):
    for of in (True, False):
        want = crop(bank.decoded("fixed", 37, of), lo, dims)
        assert differing(want, crop(bank.decoded("fixed", None, of), lo, dims)) > 0
        got = eng.decompress_box(bank.dev("fixed"), lo, dims, output_float=of, pct=37).cpu().numpy()
        assert same(got, want), (lo, dims, of)
        want = crop(bank.decoded("fixed", 10, of), lo, dims)
        got = eng.decomp_3d_portion(bank.container("fixed"), 10, box_lo_xyz=lo, box_dims_xyz=dims, output_float=of)
        assert same(got, want), (lo, dims, of)


def test_level_of_a_portion(eng, bank):
    whole = bank.oracle.decomp_3d_multi_res(bank.container("fixed"))[1]
    for pct, host in ((37, False), (10, True)):
        levels = bank.levels("fixed", pct)
        last = len(levels) - 1
        assert last > 0
        lz, ly, lx = levels[last].shape
        box = ((lx // 2 - 3, 1, lz // 2 - 1), (7, ly - 2, 3))   # across the chunk corners of x and z
        for h, lo, dims in ((0, None, None), (last, None, None), (last,) + box):
            for of in (False, True):
                want, full = levels[h], whole[h]
                if lo:
                    want, full = crop(want, lo, dims), crop(full, lo, dims)
                assert differing(want, full) > 0
                want = want.astype(np.float32) if of else want
                if host:
                    got = eng.decomp_3d_portion(bank.container("fixed"), pct, level=h, box_lo_xyz=lo, box_dims_xyz=dims,
                                                output_float=of)
                else:
                    got = eng.decompress_level(bank.dev("fixed"), h, lo, dims, output_float=of, pct=pct).cpu().numpy()
                assert same(got, want), (pct, h, lo, dims, of)


@pytest.mark.parametrize("name,pct", [("fixed", 10), ("pwe", 97), ("mixed", 20)])
def test_host_portion_decode(eng, bank, name, pct):
    for of in (True, False):
        got = eng.decomp_3d_portion(bank.container(name), pct, output_float=of)
        assert same(got, bank.decoded(name, pct, of)), (name, pct, of)
    assert same(eng.decomp_3d_portion(bank.container(name), 0), bank.decoded(name, None, True))


# ---- 4. the same kernels ------------------------------------------------------------------------------------------------

def profile_names(eng, fn):
    import torch
    torch.cuda.synchronize()
    eng.profile(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)


@pytest.mark.parametrize("name", ["fixed", "fine"])
def test_a_portion_launches_what_the_truncated_container_launches(eng, bank, name):
    cut = eng.truncate(bank.dev(name), 37)
    a = profile_names(eng, lambda: eng.decompress(bank.dev(name), True, pct=37))
    b = profile_names(eng, lambda: eng.decompress(cut, True))
    print(sum(a.values()), a)
    assert a == b and "k_trunc_container" not in a
    assert profile_names(eng, lambda: eng.truncate(bank.dev(name), 37)) == {"k_gather_heads": 1, "k_gather_bytes": 1,
                                                                           "k_trunc_container": 1}


# ---- 5. refusals leave the output as it was -------------------------------------------------------------------------------

def pattern(n):
    import torch
    return torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")


def untouched(t):
    return bool((t == 0xA5).all().item())


def test_truncate_refusals(eng, bank):
    import torch
    lib, dev, want = eng.lib, bank.dev("fixed"), bank.trunc("fixed", 37)
    n = _sz(0)
    out = pattern(len(want))
    assert lib.sperrhip_trunc_dev(dev.data_ptr(), dev.numel(), 37, out.data_ptr(), len(want) - 1, C.byref(n), None) == 1
    assert n.value == len(want) and untouched(out)
    n = _sz(0)
    assert lib.sperrhip_trunc_dev(dev.data_ptr(), dev.numel(), 37, None, 0, C.byref(n), None) == 1
    assert n.value == len(want)
    assert lib.sperrhip_trunc_dev(dev.data_ptr(), dev.numel(), 37, out.data_ptr(), len(want), C.byref(n), None) == 0
    assert host_of(out) == want
    # the source one byte short; no source
    out = pattern(dev.numel())
    assert lib.sperrhip_trunc_dev(dev.data_ptr(), dev.numel() - 1, 37, out.data_ptr(), out.numel(), C.byref(n), None) == -1
    assert lib.sperrhip_trunc_dev(None, dev.numel(), 37, out.data_ptr(), out.numel(), C.byref(n), None) == -1
    assert untouched(out)
    # ranges that overlap: the destination starts inside the source, or ends inside it
    buf = torch.cat([pattern(64), dev, pattern(dev.numel())])
    before = buf.clone()
    src = buf[64:64 + dev.numel()]
    for dst in (buf[64 + 100:], buf[64 + dev.numel() - 1:], buf[:]):
        assert lib.sperrhip_trunc_dev(src.data_ptr(), src.numel(), 37, dst.data_ptr(), dst.numel(), C.byref(n), None) == -1
        assert torch.equal(buf, before)
    dst = buf[64 + dev.numel():]   # right behind the source: fine
    assert lib.sperrhip_trunc_dev(src.data_ptr(), src.numel(), 37, dst.data_ptr(), dst.numel(), C.byref(n), None) == 0
    assert host_of(dst[:n.value]) == want and torch.equal(buf[:64 + dev.numel()], before[:64 + dev.numel()])
    # a batch: decreasing offsets, no containers
    offs, outs = (_sz * 3)(0, dev.numel(), dev.numel() - 1), (_sz * 3)()
    out = pattern(2 * dev.numel())
    assert lib.sperrhip_trunc_batch_dev(dev.data_ptr(), offs, 2, 37, out.data_ptr(), out.numel(), outs, None) == -1
    assert lib.sperrhip_trunc_batch_dev(dev.data_ptr(), offs, 0, 37, out.data_ptr(), out.numel(), outs, None) == -1
    assert untouched(out)


def test_portion_decode_refusals(eng, bank):
    lib = eng.lib
    three = _sz * 3

    def call(dev, pct, level, lo, dims, out, cap=None):
        return lib.sperrhip_decompress_portion_dev(dev.data_ptr(), dev.numel(), pct, 1,
                                                   None if level is None else C.byref(_sz(level)),
                                                   three(*lo) if lo else None, three(*dims) if dims else None,
                                                   out.data_ptr(), out.numel() if cap is None else cap, None)

    out = pattern(64 * 64 * 64 * 4)
    fixed, ragged = bank.dev("fixed"), bank.dev("ragged")
    assert call(ragged, 40, 0, None, None, out) == -1                        # the ragged container has no levels
    assert call(fixed, 37, 9, None, None, out) == -1                         # no such level
    assert call(fixed, 37, None, (60, 0, 0), (5, 1, 1), out) == -1           # a box that leaves the volume
    assert call(fixed, 37, 0, (0, 0, 0), (64, 1, 1), out) == -1              # ... that leaves the level
    assert call(fixed, 37, None, (0, 0, 0), None, out) == -1                 # half a box
    assert call(fixed, 37, None, None, (1, 1, 1), out) == -1
    assert call(fixed, 37, 0, (0, 0, 0), None, out) == -1
    assert call(fixed, 37, None, None, None, out, cap=out.numel() - 1) == -1   # an output that is too small
    assert call(fixed, 37, None, (0, 0, 0), (8, 8, 8), out, cap=8 * 8 * 8 * 4 - 1) == -1
    assert call(fixed[:-1], 37, None, None, None, out) == -1                 # a damaged container
    assert untouched(out)
    with pytest.raises(Exception):
        eng.decomp_3d_portion(bank.container("fixed"), 37, box_lo_xyz=(60, 0, 0), box_dims_xyz=(5, 1, 1))
    with pytest.raises(Exception):
        eng.decomp_3d_portion(bank.container("ragged"), 37, level=0)
    assert call(fixed, 37, None, None, None, out) == 0
    assert same(out.cpu().numpy().view(np.float32).reshape(64, 64, 64), bank.decoded("fixed", 37, True))
