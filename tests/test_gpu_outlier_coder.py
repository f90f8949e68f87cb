"""The 1D coder of the outlier list (sperr_amd/csrc/outlier.hip) beyond what containers of natural fields give it (-m gpu).

Through the public calls an outlier stream has one to three bit planes: with q = 1.5 tol the reconstruction misses by a
few tolerances at the most.  Here the decoder gets oracle containers whose outlier streams are replaced by streams of
the case table (tests/outlier_cases.py: up to 64 planes, every position found, one value per plane, the first and the
last position, runs across word boundaries), and the encoder is entered behind its reconstruction
(sperrhip_outlier_encode_dev) with errors of up to 2^62 tolerances, every integer width the reference picks and its
wrap.  The yardstick is the oracle, which tests/test_oracle_vs_ref.py::test_outlier_coder_bit_exact pins to the
reference's Outlier_Coder on the same table."""
import numpy as np
import pytest

import outlier_cases as oc
from fields import _white, smooth_field
from sperr_amd.api import SperrHipError
from sperr_amd.farm import split_container

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -10   # the containers' tolerance; their fields stay below 4 in magnitude


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
    return cuda(np.frombuffer(container, dtype=np.uint8).copy())


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def field(shape, seed=7):
    """float64, below 4 in magnitude, exact; white noise for the tiny shapes (never a constant chunk)"""
    if int(np.prod(shape)) < 64:
        return _white(shape, seed) * 2.0
    return smooth_field(shape, seed=seed, dtype=np.float64) * 2.0 ** -12


_BASE = {}


def base_of(oracle, n):
    """(a one-chunk oracle mode-3 container of the shape of n with its outlier stream cut off, its fp64 decode)"""
    if n not in _BASE:
        shape = oc.SHAPE_OF_N[n]
        v = field(shape)
        assert np.abs(v).max() <= 4.0 and v.min() != v.max()
        c = oc.graft(oracle.comp_3d(v, shape[::-1], 3, TOL), {0: b""})
        base = oracle.decomp_3d(c, False)
        base.setflags(write=False)
        _BASE[n] = (c, base)
    return _BASE[n]


# ---- decoder: crafted containers --------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n", oc.coder_cases())
def test_decoder_on_table_streams(eng, oracle, name, n):
    """One chunk whose outlier stream is the table's: both decodes have the oracle's bits, and the fp64 one differs
    from the decode without the stream by the correctors worked out in numpy -- exactly on the support, with the
    signs, 1.1 tol for a magnitude of 1 and (m - 0.25) tol otherwise to a relative 1e-9 (one fp64 add of a corrector e
    to a base b rounds by at most 2^-52 (|b| / |e| + 1) <= 2^-40 of e here: |b| <= 4 + tol, |e| >= 1.1 * 2^-10)."""
    c, base = base_of(oracle, n)
    coef, sign = oc.coder_case(name, n)
    stream = oracle.speck1d_encode(coef, sign)
    assert oc.planes_of(stream) == int(coef.max()).bit_length()
    g = oc.graft(c, {0: stream})
    dev = dev_of(g)
    got = eng.decompress(dev, False).cpu().numpy()
    assert same(got, oracle.decomp_3d(g, False))
    assert same(eng.decompress(dev, True).cpu().numpy(), oracle.decomp_3d(g, True))
    d = (got - base).reshape(-1)
    want = oc.corrector(coef, sign, TOL)
    assert np.array_equal(d != 0, coef != 0)
    assert np.array_equal(d[coef != 0] > 0, sign[coef != 0])
    assert np.all(np.abs(d - want) <= 1e-9 * np.abs(want))


MULTI = (None, "constant", "one_top", "all_one", "dense_wide", "every_plane", "single_one", "run")


def multi_container(oracle):
    """(32^3 in 16^3 chunks -- one sub-batch of eight --, each chunk with another case, so that the longest stream,
    the most planes and the most values found come from different chunks; the natural container of the same field)"""
    v = field((32, 32, 32), seed=9)
    v[:16, :16, 16:] = 0.75   # chunk 1 (x fastest)
    natural = oracle.comp_3d(v, (16, 16, 16), 3, TOL)
    parts = split_container(natural)[3]
    assert len(parts) == 8 and [len(p) == 17 for p in parts] == [k == 1 for k in range(8)]
    streams = {}
    for k, name in enumerate(MULTI):
        if name == "constant":
            continue
        streams[k] = b"" if name is None else oracle.speck1d_encode(*oc.coder_case(name, 4096))
    return oc.graft(natural, streams), natural, streams


def crop(a, lo, dims):
    return np.ascontiguousarray(a[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])


def test_decoder_multi_chunk(eng, oracle):
    """Chunks of one sub-batch with different plane counts, stream lengths and numbers of values found (maxBits,
    maxNbp, kStride and planeStride are decided by different chunks), a chunk without a stream and a constant one:
    whole, as boxes, in a batch beside a natural container, through the host call, and truncated."""
    g, natural, streams = multi_container(oracle)
    planes = {k: oc.planes_of(s) for k, s in streams.items() if s}
    assert max(planes, key=planes.get) != max(streams, key=lambda k: len(streams[k]))
    dev = dev_of(g)
    for of in (False, True):
        want = oracle.decomp_3d(g, of)
        assert same(eng.decompress(dev, of).cpu().numpy(), want), of
        for lo, dims in (((8, 8, 8), (16, 16, 16)), ((2, 18, 3), (9, 7, 5))):   # all eight chunks; inside chunk 2
            assert same(eng.decompress_box(dev, lo, dims, of).cpu().numpy(), crop(want, lo, dims)), (of, lo)
        assert same(eng.decomp_3d(g, of), want), of
        nat = oracle.decomp_3d(natural, of)
        for pair, ref in (((g, natural), (want, nat)), ((natural, g), (nat, want))):
            got = eng.decompress_batch([dev_of(p) for p in pair], of).cpu().numpy()
            assert same(got[0], ref[0]) and same(got[1], ref[1]), of
    inside = 0
    for pct in (50, 97):
        t = oracle.trunc_3d(g, pct)
        for full, cut in zip(split_container(g)[3], split_container(t)[3]):
            inside += len(full) > 17 and oc.speck_end(full) < len(cut) < len(full)
        for of in (False, True):
            assert same(eng.decompress(dev, of, pct=pct).cpu().numpy(), oracle.decomp_3d(t, of)), (pct, of)
    assert inside > 0, "no cut falls inside a crafted outlier stream"


@pytest.mark.parametrize("name", ["width_edges", "dense_wide"])
def test_decoder_2d(eng, oracle, name):
    img = field((1, 37, 50), seed=13)[0]
    stream = oracle.comp_2d(img, 3, TOL, False)
    coef, sign = oc.coder_case(name, img.size)
    g = oc.graft_2d(stream, oracle.speck1d_encode(coef, sign))
    other = oc.graft_2d(stream, b"")
    for of in (False, True):
        want = oracle.decomp_2d(g, img.shape, of)
        assert same(eng.decompress_2d(dev_of(g), img.shape, of).cpu().numpy(), want), of
        got = eng.decompress_2d_batch([dev_of(other), dev_of(g), dev_of(stream)], img.shape, of).cpu().numpy()
        assert same(got[1], want) and same(got[0], oracle.decomp_2d(other, img.shape, of)), of
        assert same(got[2], oracle.decomp_2d(stream, img.shape, of)), of
    d = oracle.decomp_2d(g, img.shape, False) - oracle.decomp_2d(other, img.shape, False)
    assert np.array_equal(d.reshape(-1) != 0, coef != 0)


def test_decoder_refuses_or_decodes_damaged_outlier_streams(eng, oracle):
    """An outlier header that claims 65 or 255 planes, and a crafted stream cut in its middle with the chunk's length
    reduced to match: rejected, or decoded as the oracle decodes it (a cut stream counts as absent,
    src/SPECK_FLT.cpp:88-103); the undamaged container decodes as before on the same engine."""
    c, _ = base_of(oracle, 4096)
    stream = oracle.speck1d_encode(*oc.coder_case("every_plane", 4096))
    good = oc.graft(c, {0: stream})
    want = oracle.decomp_3d(good, False)
    assert same(eng.decompress(dev_of(good), False).cpu().numpy(), want)
    damaged = [oc.graft(c, {0: bytes([planes]) + stream[1:]}) for planes in (65, 255)]
    damaged.append(oc.graft(c, {0: stream[:len(stream) // 2]}))
    rejected = 0
    for bad in damaged:
        try:
            got = eng.decompress(dev_of(bad), False, shape_zyx=(16, 16, 16)).cpu().numpy()
        except SperrHipError:
            rejected += 1
            continue
        assert same(got, oracle.decomp_3d(bad, False))
    assert rejected >= 2   # (more than kMaxPlanes planes is refused before anything is sized from the header)
    assert same(eng.decompress(dev_of(good), False).cpu().numpy(), want)


# ---- encoder: the production stage behind a reconstruction of the test's ------------------------------------------

def encode(eng, err, n, tol, dtype=np.float64, shape=None):
    recon, orig = oc.recon_and_orig(err, tol, dtype)
    shape = shape or oc.SHAPE_OF_N[n]
    nch = err.size // n
    stack = (shape[0] * nch,) + tuple(shape[1:])
    return eng.outlier_encode(cuda(orig.reshape(stack)), cuda(recon.reshape(stack)), shape, tol)


def oracle_stream(oracle, err, n, tol):
    pos, e = oc.outlier_list(err, tol)
    return oracle.outlier_encode(pos, e, n, tol) if pos.size else b""


ENC_TABLE = [(name, n) for name, n in oc.coder_cases() if name != "top_bit"]   # (2^63 tolerances: no error holds it)


@pytest.mark.parametrize("name,n", ENC_TABLE)
def test_encoder_on_table_cases(eng, oracle, name, n):
    """orig = recon + sign m tol, exact (1.25 tol for m = 1: an error of tol is no outlier), tol = 1: the stream is the
    oracle's of err = orig - recon, the one subtraction the kernel does; float input too where orig is exact in it"""
    coef, sign = oc.coder_case(name, n)
    err = oc.errors_of(coef, sign, 1.0)
    want = oracle_stream(oracle, err, n, 1.0)
    assert want == oracle.speck1d_encode(coef, sign)   # (no wrap at tol = 1: the width comes from the magnitudes)
    assert encode(eng, err, n, 1.0) == [want]
    if int(coef.max()) < 1 << 23:
        assert encode(eng, err, n, 1.0, np.float32) == [want]


ENC_CASES = {c[0]: c for c in oc.encoder_cases()}


@pytest.mark.parametrize("name", list(ENC_CASES))
def test_encoder_on_error_cases(eng, oracle, name):
    """the integer widths 8 to 64 with magnitudes that wrap, some or all of them to zero; ties of the rounding; the
    tolerance's boundary"""
    _, n, tol, err = ENC_CASES[name]
    want = oracle_stream(oracle, err, n, tol)
    assert encode(eng, err, n, tol) == [want]
    if name == "all_wrap_to_zero":
        assert want == bytes(9)


def test_encoder_refuses_a_raw_error_of_2_to_63(eng, oracle):
    name, n, tol, p, e = oc.REFUSED_ENCODER_CASE
    err = np.zeros(n)
    err[p] = e
    with pytest.raises(SperrHipError):
        encode(eng, err, n, tol)
    err[p] = np.nextafter(e, 0.0)
    assert encode(eng, err, n, tol) == [oracle_stream(oracle, err, n, tol)]


def test_encoder_six_chunks_in_one_call(eng, oracle):
    """kmax, maxPlanes and the sparse / dense bound of the stream come from different chunks; then a call with the
    first chunk alone, and with the dense one alone, on the buffers the large call left"""
    n, tol = 4096, TOL
    zero = np.zeros(n)
    zero[oc._hashed(n, 50, 73)] = (np.arange(50) + 1) * 256 * tol   # every magnitude a multiple of 256 under uint8
    quiet = np.zeros(n)
    quiet[5], quiet[77] = tol, -0.5 * tol   # nothing beyond the tolerance
    errs = [quiet]
    for name in ("one_top", "all_one", "dense_wide"):
        errs.append(oc.errors_of(*oc.coder_case(name, n), tol))
    errs.append(zero)
    errs.append(oc.errors_of(*oc.coder_case("every_plane", n), tol))
    want = [oracle_stream(oracle, e, n, tol) for e in errs]
    assert want[0] == b"" and want[4] == bytes(9) and want[1][0] == 63 and want[5][0] == 63
    assert max(range(6), key=lambda k: len(want[k])) not in (1, 5)   # the longest stream is not the deepest one
    assert encode(eng, np.concatenate(errs), n, tol) == want
    assert encode(eng, errs[0], n, tol) == [b""]
    assert encode(eng, errs[3], n, tol) == [want[3]]
    assert encode(eng, np.concatenate(errs[::-1]), n, tol) == want[::-1]


@pytest.mark.parametrize("name", ["run", "dense_wide", "every_plane"])
def test_round_trip_through_a_container(eng, oracle, name):
    """the GPU's stream grafted into a container and decoded on the GPU is the oracle's decode of the oracle's"""
    n = 8190
    c, _ = base_of(oracle, n)
    err = oc.errors_of(*oc.coder_case(name, n), TOL)
    ours = encode(eng, err, n, TOL)[0]
    theirs = oracle_stream(oracle, err, n, TOL)
    for of in (False, True):
        got = eng.decompress(dev_of(oc.graft(c, {0: ours})), of).cpu().numpy()
        assert same(got, oracle.decomp_3d(oc.graft(c, {0: theirs}), of)), of
