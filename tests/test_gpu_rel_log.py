"""GPU: the LOG map kind of point-wise relative error (include/sperr_hip.h "relative error", sperr_amd/csrc/rel.h,
rel_log.hip, abi_rel.hip): map="log" on rel_tolerance, rel_forward and compress_rel, the *_kind entry points under them,
and the decodes, which take the kind from the side stream's magic "SPLG".

Every comparison is bit for bit, through integer views; tests/rel_log_model.py is the numpy statement of the kind, built
from the same IEEE operations in the same order, so the device's y and x' are its bits.

  volumes      test_gpu_rel.py's six: ragged tiles, chunk edges, the planted adversarial samples, fp32 and fp64
  rel_forward  y, the side stream and the counts are the model's, with the source at element 0 and 1 of its allocation
  compress_rel the container is compress_masked's of the model's y in mode 3 at the model's t for the three fills, the
               side stream is the model's; with the midrange fill the oracle makes the same bytes and decodes them
  decompress_rel  the model's inverse of the dense double decode: whole and a box, float and double output, between
               guard bytes; rel_inverse in place on doubles
  guarantee    |y' - y| <= t, then rel_check: no violation, no class mismatch, its figures numpy's
  smaller      on the two chunked vort cases the log container is smaller than the linear kind's for the same eps
  pct=25       finite, zeros and signs exact
  mixed kinds  an SPLG stream with a linear-kind container decodes (the payload is trusted); a broken magic, an
               unknown kind and a small side_cap are refused or answered with every output as it was
  states       one pair behind pending work on a side stream; one pair in a fresh child process on a poisoned workspace"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mask_model as M
import rel_log_model as L
import rel_model as R
from test_gpu_rel import FILLS, GUARD, VOLUMES, dev_at, guarded, same_bits

pytestmark = pytest.mark.gpu

_sz = C.c_size_t


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    yield e
    e.release()


class Case:
    """a volume, the log kind's model of it, and what the library made of it: computed once, shared, left unchanged"""

    def __init__(self, eng, name):
        import torch
        make, self.chunks, self.eps, self.box_lo, self.box_dims = VOLUMES[name]
        self.vol = make()
        self.is_float = self.vol.dtype == np.float32
        self.t = L.tolerance(self.eps, self.is_float)
        self.y, self.zero, self.neg = L.forward(self.vol)
        self.side_want = L.side_stream(self.zero, self.neg, self.eps, self.is_float)
        self.dev = torch.from_numpy(self.vol).cuda()
        self.container, self.side = eng.compress_rel(self.dev, self.chunks, self.eps, map="log")
        self.yp = eng.decompress(self.container, output_float=False).cpu().numpy()   # the dense double decode

    def box(self, a):
        (x, y, z), (bx, by, bz) = self.box_lo, self.box_dims
        return np.ascontiguousarray(a.reshape(self.vol.shape)[z:z + bz, y:y + by, x:x + bx])

    def want(self, output_float, box=False, yp=None):
        pick = self.box if box else (lambda a: a.reshape(self.vol.shape))
        return L.inverse(pick(self.yp if yp is None else yp), pick(self.zero), pick(self.neg), output_float,
                         self.is_float)


_cases = {}


def get_case(eng, name):
    if name not in _cases:
        _cases[name] = Case(eng, name)
    return _cases[name]


@pytest.fixture(params=list(VOLUMES))
def case(request, eng):
    return get_case(eng, request.param)


@pytest.mark.parametrize("lead", [0, 1])
def test_rel_forward_log_is_the_models(eng, case, lead):
    src = dev_at(case.vol, lead)
    y, side, nzero, nneg = eng.rel_forward(src, map="log")
    assert same_bits(y.cpu().numpy(), case.y)
    assert bytes(side.cpu().numpy()) == L.side_stream(case.zero, case.neg, 0.0, case.is_float)
    assert (nzero, nneg) == (int(case.zero.sum()), int(case.neg.sum()))
    assert eng.rel_parse(side) == (case.is_float, 0.0, case.vol.size, nzero, nneg) and eng.rel_kind(side) == "log"
    assert same_bits(src.cpu().numpy(), case.vol.reshape(-1)), "the source was written"
    # the inverse of y itself: every float comes back, doubles within the two maps' rounding
    back = eng.rel_inverse(y, side, output_float=case.is_float).cpu().numpy()
    assert same_bits(back, L.inverse(case.y, case.zero, case.neg, case.is_float, case.is_float))
    nz = ~case.zero
    if case.is_float:
        assert same_bits(back[nz], case.vol.reshape(-1)[nz])
    else:
        with np.errstate(over="ignore"):
            x = case.vol.reshape(-1)[nz]
            assert (np.abs(back[nz] - x) <= 2.0 ** -43 * np.abs(x)).all()


@pytest.mark.parametrize("fill", list(FILLS))
def test_compress_rel_log_is_compress_masked_of_the_models_y(eng, oracle, case, fill):
    import torch
    container, side = (case.container, case.side) if fill == "smooth" else eng.compress_rel(
        case.dev, case.chunks, case.eps, fill=FILLS[fill], map="log")
    assert eng.rel_tolerance(case.eps, case.is_float, map="log") == case.t
    yd = torch.from_numpy(case.y.reshape(case.vol.shape)).cuda()
    want, zmask = eng.compress_masked(yd, case.chunks, case.t, mode=3, missing="nan", fill=FILLS[fill])
    got = bytes(container.cpu().numpy())
    assert got == bytes(want.cpu().numpy())
    s = bytes(side.cpu().numpy())
    assert s == case.side_want and len(s) <= eng.rel_max_size(case.vol.size)
    assert s[48:48 + len(zmask)] == bytes(zmask.cpu().numpy())
    assert eng.rel_parse(side) == (case.is_float, case.eps, case.vol.size, int(case.zero.sum()), int(case.neg.sum()))
    assert eng.rel_kind(side) == "log"
    assert eng.parse_header(container)[0] == case.vol.shape
    if fill == "midrange":
        shape = case.vol.shape
        assert got == oracle.comp_3d(M.filled(case.y.reshape(shape), case.zero.reshape(shape)), case.chunks, 3, case.t)
        assert same_bits(oracle.decomp_3d(got, output_float=False),
                         eng.decompress(container, output_float=False).cpu().numpy())


@pytest.mark.parametrize("output_float", [True, False], ids=["float", "double"])
@pytest.mark.parametrize("box", [False, True], ids=["whole", "box"])
def test_decompress_rel_is_the_log_models_inverse_of_the_dense_decode(eng, case, box, output_float):
    import torch
    want = case.want(output_float, box)
    kw = dict(box_lo_xyz=case.box_lo, box_dims_xyz=case.box_dims) if box else {}
    out, buf = guarded(want.shape, torch.float32 if output_float else torch.float64)
    back = eng.decompress_rel(case.container, case.side, output_float=output_float, out=out, **kw)
    assert back.data_ptr() == out.data_ptr() and same_bits(out.cpu().numpy(), want)
    edge = buf.cpu().numpy()
    assert (edge[:GUARD] == -777.0).all() and (edge[-GUARD:] == -777.0).all(), "guard bytes were written"
    if not output_float:   # rel_inverse in place on the doubles of the dense decode
        yd = torch.from_numpy(case.box(case.yp) if box else case.yp.copy()).cuda()
        same = eng.rel_inverse(yd, case.side, output_float=False, out=yd, vol_shape_zyx=case.vol.shape, **kw)
        assert same.data_ptr() == yd.data_ptr() and same_bits(yd.cpu().numpy(), want)


def test_the_guarantee(eng, case):
    nz = ~case.zero
    gap = np.abs(case.yp.reshape(-1)[nz] - case.y[nz])
    print(f"largest |y' - y| {gap.max():.6e} of t {case.t:.6e}; {case.container.numel()} + {case.side.numel()} bytes "
          f"for {case.vol.nbytes}")
    assert (gap <= case.t).all(), "the coder's own point-wise bound"
    for output_float in ((True, False) if case.is_float else (False,)):
        recon = eng.decompress_rel(case.container, case.side, output_float=output_float)
        orig = case.dev if recon.dtype == case.dev.dtype else case.dev.to(recon.dtype)   # (float -> double is exact)
        got = eng.rel_check(orig, recon, case.eps)
        want = R.check(orig.cpu().numpy(), recon.cpu().numpy(), case.eps)
        print(f"float output {output_float}: worst |x' - x| / |x| {got[0]:.6e} of eps {case.eps}")
        assert got == want, (got, want)
        assert got[1] == 0 and got[2] == 0 and got[3] == int(nz.sum())


@pytest.mark.parametrize("name", ["vort_chunks", "vort_chunks_1e-4"])
def test_the_log_container_is_smaller_than_the_linear_kinds(eng, name):
    case = get_case(eng, name)
    linear, side = eng.compress_rel(case.dev, case.chunks, case.eps)
    print(f"{name}: log {case.container.numel()} bytes, linear {linear.numel()}")
    assert eng.rel_kind(side) == "linear" and bytes(side.cpu().numpy())[4:] == case.side_want[4:]
    assert case.container.numel() < linear.numel()


def test_a_portion_is_finite_with_exact_zeros_and_signs(eng, case):
    for output_float in (True, False):
        got = eng.decompress_rel(case.container, case.side, pct=25, output_float=output_float).cpu().numpy()
        assert np.isfinite(got).all()
        assert np.array_equal(np.signbit(got.reshape(-1)), case.neg) and (got.reshape(-1)[case.zero] == 0).all()
        yp = eng.decompress(case.container, output_float=False, pct=25).cpu().numpy()
        assert same_bits(got, case.want(output_float, yp=yp))


def test_mixed_kinds_and_refusals_leave_every_output_as_it_was(eng):
    import torch
    case = get_case(eng, "cube17")
    vol, dims = case.vol, tuple(reversed(case.vol.shape))
    n = vol.size
    # an SPLG stream with the linear kind's container of the same volume: the payload is trusted, the map is the stream's
    linear, lin_side = eng.compress_rel(case.dev, case.chunks, case.eps)
    yp_lin = eng.decompress(linear, output_float=False).cpu().numpy()
    got = eng.decompress_rel(linear, case.side, output_float=True).cpu().numpy()
    assert same_bits(got, case.want(True, yp=yp_lin))
    got = eng.decompress_rel(case.container, lin_side, output_float=False).cpu().numpy()
    assert same_bits(got, R.inverse(case.yp, case.zero.reshape(vol.shape), case.neg.reshape(vol.shape), False, True))
    # a magic that is neither: refused, the destination untouched
    dst = torch.full((n,), -777.0, dtype=torch.float32, device="cuda")

    def decode(side_t):
        return eng.lib.sperrhip_decompress_rel_dev(case.container.data_ptr(), case.container.numel(), 0, 1, None, None,
                                                   side_t.data_ptr(), side_t.numel(), dst.data_ptr(), dst.numel() * 4,
                                                   eng._stream())

    for at, val in ((2, ord("X")), (3, ord("X")), (2, ord("R")), (3, ord("L")), (4, 2), (6, 1), (40, 1)):
        broken = case.side.clone()
        broken[at] = val
        assert decode(broken) == -1 and bool((dst == -777.0).all()), (at, val)
        with pytest.raises(Exception):
            eng.rel_kind(broken)
    assert decode(case.side) == 0 and same_bits(dst.cpu().numpy().reshape(vol.shape), case.want(True))
    # an eps between the two kinds' floors is the log kind's alone, going in and in a stream
    between = L.tolerance_floor(True)
    assert eng.rel_tolerance(between, True, map="log") == L.tolerance(between, True)
    with pytest.raises(Exception):
        eng.rel_tolerance(between, True)
    # the unknown kind 2 on the three new entry points that take one
    out = torch.full((eng.max_compressed_size(vol.shape, case.chunks, case.t, 3),), 0xA5, dtype=torch.uint8, device="cuda")
    side = torch.full((eng.rel_max_size(n),), 0x5A, dtype=torch.uint8, device="cuda")
    y = torch.full((n,), -777.0, dtype=torch.float64, device="cuda")

    def untouched():
        return bool((out == 0xA5).all()) and bool((side == 0x5A).all()) and bool((y == -777.0).all())

    def compress(kind, side_cap, eps=case.eps):
        clen, slen = _sz(12345), _sz(12345)
        rtn = eng.lib.sperrhip_compress_rel_kind_dev(case.dev.data_ptr(), 1, *dims, *case.chunks, float(eps), kind, 2,
                                                     0.0, out.data_ptr(), out.numel(), C.byref(clen), side.data_ptr(),
                                                     side_cap, C.byref(slen), eng._stream())
        return rtn, clen.value, slen.value

    def forward(kind, side_cap):
        slen, nzero, nneg = _sz(12345), _sz(12345), _sz(12345)
        rtn = eng.lib.sperrhip_rel_forward_kind_dev(case.dev.data_ptr(), 1, n, kind, y.data_ptr(), side.data_ptr(),
                                                    side_cap, C.byref(slen), C.byref(nzero), C.byref(nneg),
                                                    eng._stream())
        return rtn, slen.value, nzero.value, nneg.value

    t = C.c_double(-5.0)
    for kind in (2, -1):
        assert eng.lib.sperrhip_rel_tolerance_kind(1e-2, 1, kind, C.byref(t)) == -1 and t.value == -5.0
        assert compress(kind, side.numel()) == (-1, 12345, 12345) and untouched()
        assert forward(kind, side.numel()) == (-1, 12345, 12345, 12345) and untouched()
    with pytest.raises(ValueError):
        eng.compress_rel(case.dev, case.chunks, case.eps, map="cubic")
    # this kind's refusals of eps
    for eps in (0.0, -1e-2, 0.6, float("nan"), float("inf"), between * 0.999):
        assert compress(1, side.numel(), eps)[0] == -1 and untouched(), eps
    # side_cap one byte short: 1 and the size needed, nothing written
    need = len(case.side_want)
    rtn, _, slen = compress(1, need - 1)
    assert (rtn, slen) == (1, need) and untouched()
    rtn, slen, _, _ = forward(1, need - 1)
    assert (rtn, slen) == (1, need) and untouched()
    rtn, clen, slen = compress(1, need)
    assert (rtn, slen) == (0, need) and bytes(side[:need].cpu().numpy()) == case.side_want
    assert bytes(out[:clen].cpu().numpy()) == bytes(case.container.cpu().numpy()) and bool((side[need:] == 0x5A).all())
    # kind 0 through the new entry points is the calls without a kind
    rtn, clen, slen = compress(0, side.numel())
    assert rtn == 0 and bytes(out[:clen].cpu().numpy()) == bytes(linear.cpu().numpy())
    assert bytes(side[:slen].cpu().numpy()) == bytes(lin_side.cpu().numpy())
    kind = C.c_int(-1)
    assert eng.lib.sperrhip_rel_parse_stream_kind_dev(case.side.data_ptr(), case.side.numel(), None, None, None, None,
                                                      None, C.byref(kind), eng._stream()) == 0 and kind.value == 1


def test_a_pair_behind_pending_work_on_a_side_stream(eng):
    """the source is still being produced on a non-default stream when compress_rel is queued there, and the decode is
    queued behind the compress"""
    import torch
    case = get_case(eng, "vort_chunks")
    st = torch.cuda.Stream()
    host = torch.from_numpy(case.vol).pin_memory()
    with torch.cuda.stream(st):
        big = torch.ones(2048, 2048, device="cuda")
        for _ in range(20):   # work the stream has to get through first
            big = (big @ big) * (1.0 / 2048.0)
        src = torch.empty(case.vol.shape, dtype=torch.float32, device="cuda")
        src.copy_(host, non_blocking=True)
        src = src * 1.0   # (a kernel between the copy and the call; it keeps the sign of -0.0)
        container, side = eng.compress_rel(src, case.chunks, case.eps, map="log")
        back = eng.decompress_rel(container, side, output_float=True)
    st.synchronize()
    assert bytes(container.cpu().numpy()) == bytes(case.container.cpu().numpy())
    assert bytes(side.cpu().numpy()) == case.side_want
    assert same_bits(back.cpu().numpy(), case.want(True))


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from sperr_amd.api import SperrHip
from sperr_amd.synth import turbulence
from rel_model import vort_with_zeros
out = sys.argv[2]
eng = SperrHip()
# the call before: another chunk shape, another mode, both ways
hist = torch.from_numpy(turbulence((36, 40, 44), seed=9)).cuda()
eng.decompress(eng.compress(hist, (20, 20, 20), 3.0, mode=1))
vol = torch.from_numpy(vort_with_zeros()).cuda()
container, side = eng.compress_rel(vol, (20, 18, 16), 1e-2, map="log")
eng.decompress(eng.compress(hist, (20, 20, 20), 3.0, mode=1))
dst = torch.full((vol.numel() + 16,), -777.0, dtype=torch.float32, device="cuda")
back = eng.decompress_rel(container, side, out=dst[:vol.numel()].view(vol.shape))
box = eng.decompress_rel(container, side, box_lo_xyz=(3, 5, 7), box_dims_xyz=(21, 17, 13), output_float=False)
torch.cuda.synchronize()
assert bool((dst[vol.numel():] == -777.0).all())
container.cpu().numpy().tofile(out + "/c.bin")
side.cpu().numpy().tofile(out + "/side.bin")
back.cpu().numpy().tofile(out + "/dec.f32")
box.cpu().numpy().tofile(out + "/box.f64")
"""


def test_a_pair_on_a_poisoned_workspace_in_a_fresh_process(eng, tmp_path):
    """SPERR_HIP_POISON=0xFF for a whole child process, started as a child: the engine's buffers are filled with NaNs
    before every call carves them, behind a fixed-rate call of another chunk shape"""
    case = get_case(eng, "vort_chunks")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SPERR_HIP_POISON="0xFF")
    p = subprocess.run([sys.executable, "-c", CHILD, root, str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert (tmp_path / "c.bin").read_bytes() == bytes(case.container.cpu().numpy())
    assert (tmp_path / "side.bin").read_bytes() == case.side_want
    got = np.fromfile(tmp_path / "dec.f32", dtype=np.float32).reshape(case.vol.shape)
    assert same_bits(got, case.want(True))
    got = np.fromfile(tmp_path / "box.f64", dtype=np.float64)
    assert same_bits(got.reshape(case.want(False, box=True).shape), case.want(False, box=True))
