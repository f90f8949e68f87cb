"""GPU: point-wise relative error (include/sperr_hip.h "relative error", sperr_amd/csrc/rel.h, rel.hip, abi_rel.hip) -- a
volume becomes an ordinary container of the double volume y in point-wise error mode and a side stream with the zero
and sign bits; the decode gives |x' - x| <= eps |x| with zeros and signs exact.

Every comparison is bit for bit, through integer views; tests/rel_model.py is the numpy statement of the rule.

  volumes      tests/golden/vort_crop.f32 (33, 36, 40) with a ball of zeros and a few -0.0, whole and in chunks
               (20, 18, 16); 17^3 (4913 samples: neither a tile of 1024 nor a word of 64); a (17, 20, 24) volume spanning
               2^-140 to 2^120 with the adversarial samples planted, as fp32 and as fp64 (which adds double subnormals)
  rel_forward  y and the side stream are the model's, from a source at the start of its allocation (the 16-byte form)
               and one element into it (the element form)
  compress_rel the container and the zero stream are compress_masked's of the model's y in mode 3 at t, for the three
               fills, and with the midrange fill the oracle's of the model's in-filled y
  decompress_rel  the model's inverse of the dense double decode: whole and a box with an odd origin that cuts chunks,
               float and double output, with out= between guard bytes and without; rel_inverse in place on doubles
  guarantee    |y' - y| <= t outside the zero class (the coder's part), then rel_check: no violation, no class
               mismatch, its figures numpy's
  pct=25       finite, zeros and signs exact
  refusals     leave the container, the side buffer and the output as they were; a small side_cap returns 1 and the size
  streams      one pair behind inputs still pending on a non-default stream"""
import ctypes as C

import numpy as np
import pytest

import mask_model as M
import rel_model as R

pytestmark = pytest.mark.gpu

_sz = C.c_size_t
GUARD = 64
FILLS = {"midrange": "midrange", "smooth": "smooth", "value": 3.25}


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    yield e
    e.release()


def _ibits(a):
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_ibits(np.ascontiguousarray(a)),
                                                                        _ibits(np.ascontiguousarray(b)))


def _cube17():
    return R.planted_volume((17, 17, 17), np.float32, seed=3)


# name: (volume (z, y, x), chunks (x, y, z), eps, box lo (x, y, z), box dims (x, y, z))
VOLUMES = {
    "vort_whole": (R.vort_with_zeros, (40, 36, 33), 1e-2, (3, 5, 7), (21, 17, 13)),
    "vort_chunks": (R.vort_with_zeros, (20, 18, 16), 1e-2, (3, 5, 7), (21, 17, 13)),
    "vort_chunks_1e-4": (R.vort_with_zeros, (20, 18, 16), 1e-4, (19, 1, 15), (11, 33, 5)),
    "cube17": (_cube17, (17, 17, 17), 1e-2, (1, 3, 5), (13, 12, 9)),
    "planted_f32": (lambda: R.planted_volume((17, 20, 24), np.float32), (16, 16, 16), 1e-2, (5, 3, 1), (17, 15, 13)),
    "planted_f64": (lambda: R.planted_volume((17, 20, 24), np.float64), (16, 16, 16), 1e-2, (5, 3, 1), (17, 15, 13)),
}


class Case:
    """a volume, its model, and what the library made of it: computed once, shared and left unchanged"""

    def __init__(self, eng, name):
        import torch
        make, self.chunks, self.eps, self.box_lo, self.box_dims = VOLUMES[name]
        self.vol = make()
        self.is_float = self.vol.dtype == np.float32
        self.t = R.tolerance(self.eps, self.is_float)
        self.y, self.zero, self.neg = R.forward(self.vol)
        self.side_want = R.side_stream(self.zero, self.neg, self.eps, self.is_float)
        self.dev = torch.from_numpy(self.vol).cuda()
        self.container, self.side = eng.compress_rel(self.dev, self.chunks, self.eps)
        self.yp = eng.decompress(self.container, output_float=False).cpu().numpy()   # the dense double decode

    def box(self, a):
        (x, y, z), (bx, by, bz) = self.box_lo, self.box_dims
        return np.ascontiguousarray(a.reshape(self.vol.shape)[z:z + bz, y:y + by, x:x + bx])

    def want(self, output_float, box=False):
        pick = self.box if box else (lambda a: a.reshape(self.vol.shape))
        return R.inverse(pick(self.yp), pick(self.zero), pick(self.neg), output_float, self.is_float)


_cases = {}


@pytest.fixture(params=list(VOLUMES))
def case(request, eng):
    if request.param not in _cases:
        _cases[request.param] = Case(eng, request.param)
    return _cases[request.param]


def dev_at(a, lead):
    """the array on the device, its first element `lead` elements into an allocation"""
    import torch
    buf = torch.zeros(a.size + lead, dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[lead:] = torch.from_numpy(a.reshape(-1)).cuda()
    return buf[lead:]


@pytest.mark.parametrize("lead", [0, 1])
def test_rel_forward_is_the_models(eng, case, lead):
    src = dev_at(case.vol, lead)
    y, side, nzero, nneg = eng.rel_forward(src)
    assert same_bits(y.cpu().numpy(), case.y)
    assert bytes(side.cpu().numpy()) == R.side_stream(case.zero, case.neg, 0.0, case.is_float)
    assert (nzero, nneg) == (int(case.zero.sum()), int(case.neg.sum()))
    assert eng.rel_parse(side) == (case.is_float, 0.0, case.vol.size, nzero, nneg)
    assert same_bits(src.cpu().numpy(), case.vol.reshape(-1)), "the source was written"
    # the inverse of y itself: the samples for floats, and for doubles within the rounding of y
    back = eng.rel_inverse(y, side, output_float=case.is_float).cpu().numpy()
    assert same_bits(back, R.inverse(case.y, case.zero, case.neg, case.is_float, case.is_float))
    if case.is_float:
        nz = ~case.zero
        assert same_bits(back[nz], case.vol.reshape(-1)[nz])


@pytest.mark.parametrize("fill", list(FILLS))
def test_compress_rel_is_compress_masked_of_the_models_y(eng, oracle, case, fill):
    import torch
    container, side = (case.container, case.side) if fill == "smooth" else eng.compress_rel(case.dev, case.chunks,
                                                                                            case.eps, fill=FILLS[fill])
    yd = torch.from_numpy(case.y.reshape(case.vol.shape)).cuda()
    want, zmask = eng.compress_masked(yd, case.chunks, case.t, mode=3, missing="nan", fill=FILLS[fill])
    got = bytes(container.cpu().numpy())
    assert got == bytes(want.cpu().numpy())
    s = bytes(side.cpu().numpy())
    assert s == case.side_want and len(s) <= eng.rel_max_size(case.vol.size) == R.max_size(case.vol.size)
    assert s[48:48 + len(zmask)] == bytes(zmask.cpu().numpy())
    assert eng.rel_parse(side) == (case.is_float, case.eps, case.vol.size, int(case.zero.sum()), int(case.neg.sum()))
    assert eng.parse_header(container)[0] == case.vol.shape
    if fill == "midrange":
        shape = case.vol.shape
        assert got == oracle.comp_3d(M.filled(case.y.reshape(shape), case.zero.reshape(shape)), case.chunks, 3, case.t)


def guarded(shape, dtype):
    """(a tensor of `shape` between GUARD sentinel elements, the whole buffer)"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), -777.0, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + n].view(tuple(shape)), buf


@pytest.mark.parametrize("output_float", [True, False], ids=["float", "double"])
@pytest.mark.parametrize("box", [False, True], ids=["whole", "box"])
def test_decompress_rel_is_the_models_inverse_of_the_dense_decode(eng, case, box, output_float):
    import torch
    want = case.want(output_float, box)
    kw = dict(box_lo_xyz=case.box_lo, box_dims_xyz=case.box_dims) if box else {}
    got = eng.decompress_rel(case.container, case.side, output_float=output_float, **kw)
    assert same_bits(got.cpu().numpy(), want)
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
    import torch
    nz = ~case.zero
    gap = np.abs(case.yp.reshape(-1)[nz] - case.y[nz])
    print(f"largest |y' - y| {gap.max():.6e} of t {case.t:.6e}; {len(bytes(case.container.cpu().numpy()))} + "
          f"{case.side.numel()} bytes for {case.vol.nbytes}")
    assert (gap <= case.t).all(), "the coder's own point-wise bound"
    for output_float in ((True, False) if case.is_float else (False,)):
        recon = eng.decompress_rel(case.container, case.side, output_float=output_float)
        orig = case.dev if recon.dtype == case.dev.dtype else case.dev.to(recon.dtype)   # (float -> double is exact)
        got = eng.rel_check(orig, recon, case.eps)
        want = R.check(orig.cpu().numpy(), recon.cpu().numpy(), case.eps)
        print(f"float output {output_float}: worst |x' - x| / |x| {got[0]:.6e} of eps {case.eps}")
        assert got == want, (got, want)
        assert got[1] == 0 and got[2] == 0 and got[3] == int(nz.sum())
    # the check sees what is wrong: a sign, a zero made nonzero, a sample moved past the bound
    recon = eng.decompress_rel(case.container, case.side, output_float=case.is_float).clone()
    flat = recon.view(-1)
    i_nz, i_z = int(np.flatnonzero(nz)[0]), int(np.flatnonzero(case.zero)[0])
    flat[i_nz] = -flat[i_nz]
    flat[i_z] = 1.0
    j = int(np.flatnonzero(nz)[1])
    flat[j] = flat[j] * (1.0 + 3.0 * case.eps)
    got = eng.rel_check(case.dev, recon, case.eps)
    assert got == R.check(case.vol, recon.cpu().numpy(), case.eps) and got[1] == 2 and got[2] == 2


def test_a_portion_is_finite_with_exact_zeros_and_signs(eng, case):
    for output_float in (True, False):
        got = eng.decompress_rel(case.container, case.side, pct=25, output_float=output_float).cpu().numpy().reshape(-1)
        assert np.isfinite(got).all()
        assert np.array_equal(np.signbit(got), case.neg) and (got[case.zero] == 0).all()
        yp = eng.decompress(case.container, output_float=False, pct=25).cpu().numpy()
        assert same_bits(got.reshape(case.vol.shape),
                         R.inverse(yp, case.zero, case.neg, output_float, case.is_float).reshape(case.vol.shape))


def _call_compress(eng, src, dims_xyz, chunks, eps, fill, out, side, side_cap=None):
    n, slen = _sz(0), _sz(0)
    rtn = eng.lib.sperrhip_compress_rel_dev(src.data_ptr() if src is not None else None, int(src.element_size() == 4)
                                            if src is not None else 1, *dims_xyz, *chunks, float(eps), fill, 0.0,
                                            out.data_ptr(), out.numel(), C.byref(n), side.data_ptr(),
                                            side.numel() if side_cap is None else side_cap, C.byref(slen),
                                            eng._stream())
    return rtn, n.value, slen.value


def test_refusals_leave_every_output_as_it_was(eng):
    import torch
    case = _cases.get("cube17") or Case(eng, "cube17")
    vol, dims = case.vol, tuple(reversed(case.vol.shape))
    n = vol.size
    out = torch.full((eng.max_compressed_size(vol.shape, case.chunks, case.t, 3),), 0xA5, dtype=torch.uint8, device="cuda")
    side = torch.full((eng.rel_max_size(n),), 0x5A, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool((out == 0xA5).all()) and bool((side == 0x5A).all())

    # compress: eps, a sample that is not finite, NULL, n of 0, an unknown fill
    for eps in (0.0, -1e-2, 0.6, float("nan"), float("inf"), R.tolerance_floor(True) * 0.999):
        assert _call_compress(eng, case.dev, dims, case.chunks, eps, 2, out, side)[0] == -1 and untouched(), eps
    for bad in (np.inf, -np.inf, np.nan):
        v = vol.copy()
        v.reshape(-1)[n - 3] = bad
        assert _call_compress(eng, torch.from_numpy(v).cuda(), dims, case.chunks, 1e-2, 2, out, side)[0] == -1
        assert untouched(), bad
    assert _call_compress(eng, None, dims, case.chunks, 1e-2, 2, out, side)[0] == -1 and untouched()
    assert _call_compress(eng, case.dev, (0, 17, 17), case.chunks, 1e-2, 2, out, side)[0] == -1 and untouched()
    assert _call_compress(eng, case.dev, dims, case.chunks, 1e-2, 7, out, side)[0] == -1 and untouched()
    with pytest.raises(Exception):
        eng.compress_rel(case.dev, case.chunks, 0.6)
    # side_cap too small: 1, the size needed, nothing written
    need = len(case.side_want)
    rtn, _, slen = _call_compress(eng, case.dev, dims, case.chunks, case.eps, 2, out, side, side_cap=need - 1)
    assert (rtn, slen) == (1, need) and untouched()
    rtn, clen, slen = _call_compress(eng, case.dev, dims, case.chunks, case.eps, 2, out, side, side_cap=need)
    assert (rtn, slen) == (0, need) and bytes(side[:need].cpu().numpy()) == case.side_want
    assert bytes(out[:clen].cpu().numpy()) == bytes(case.container.cpu().numpy())
    assert bool((side[need:] == 0x5A).all())
    # forward: the same for y and the side buffer
    y = torch.full((n,), -777.0, dtype=torch.float64, device="cuda")
    side.fill_(0x5A)
    v = vol.copy()
    v.reshape(-1)[1] = np.nan
    slen, nzero, nneg = _sz(0), _sz(0), _sz(0)

    def forward(src, cap):
        return eng.lib.sperrhip_rel_forward_dev(src.data_ptr(), 1, n, y.data_ptr(), side.data_ptr(), cap, C.byref(slen),
                                                C.byref(nzero), C.byref(nneg), eng._stream())

    assert forward(torch.from_numpy(v).cuda(), side.numel()) == -1
    assert bool((y == -777.0).all()) and bool((side == 0x5A).all())
    assert forward(case.dev, need - 1) == 1 and slen.value == need
    assert bool((y == -777.0).all()) and bool((side == 0x5A).all())
    # decode: a refused side stream, n against the container, a float container, a box that leaves the volume, a
    # destination that is too small
    dst = torch.full((n,), -777.0, dtype=torch.float32, device="cuda")

    def decode(container, side_t, lo=None, dims_=None, cap=None):
        lo_c = (_sz * 3)(*lo) if lo is not None else None
        dm_c = (_sz * 3)(*dims_) if dims_ is not None else None
        return eng.lib.sperrhip_decompress_rel_dev(container.data_ptr(), container.numel(), 0, 1, lo_c, dm_c,
                                                   side_t.data_ptr(), side_t.numel(), dst.data_ptr(),
                                                   dst.numel() * 4 if cap is None else cap, eng._stream())

    good = case.side
    for at, val in ((0, ord("X")), (4, 2), (5, 7), (6, 1), (40, 1), (24, 8), (48, ord("X")), (48 + 5, 3)):
        broken = good.clone()
        broken[at] = val
        assert decode(case.container, broken) == -1 and bool((dst == -777.0).all()), at
    sign_at = 48 + (int.from_bytes(case.side_want[24:32], "little") + 7) // 8 * 8
    broken = good.clone()
    broken[sign_at + 1] = ord("X")
    assert decode(case.container, broken) == -1 and bool((dst == -777.0).all())
    assert decode(case.container, good[:-4].clone()) == -1 and bool((dst == -777.0).all())
    other = _cases.get("vort_whole") or Case(eng, "vort_whole")
    assert decode(case.container, other.side) == -1 and bool((dst == -777.0).all())          # n
    ramp = torch.linspace(1.0, 2.0, n, dtype=torch.float32, device="cuda").view(vol.shape)
    as_float = eng.compress(ramp, case.chunks, 1e-3, mode=3)
    assert decode(as_float, good) == -1 and bool((dst == -777.0).all())                     # not a double container
    assert decode(case.container, good, (10, 0, 0), (8, 17, 17)) == -1 and bool((dst == -777.0).all())
    assert decode(case.container, good, (0, 0, 0), (0, 17, 17)) == -1 and bool((dst == -777.0).all())
    assert decode(case.container, good, cap=n * 4 - 1) == -1 and bool((dst == -777.0).all())
    assert decode(case.container, good) == 0 and same_bits(dst.cpu().numpy().reshape(vol.shape), case.want(True))
    # the inverse alone: n against the stream's, a float output in place
    yd = torch.from_numpy(case.yp.copy()).cuda()
    with pytest.raises(Exception):
        eng.rel_inverse(yd.view(-1)[:-1].clone(), good, output_float=False)
    vd = (_sz * 3)(n, 1, 1)
    assert eng.lib.sperrhip_rel_inverse_dev(yd.data_ptr(), vd, None, None, good.data_ptr(), good.numel(), 1,
                                            yd.data_ptr(), eng._stream()) == -1
    assert same_bits(yd.cpu().numpy(), case.yp)
    # the check
    out4 = (C.c_double * 4)()
    for eps in (-1.0, float("nan"), float("inf")):
        assert eng.lib.sperrhip_rel_check_dev(case.dev.data_ptr(), case.dev.data_ptr(), 1, n, eps, out4,
                                              eng._stream()) == -1
    assert eng.lib.sperrhip_rel_check_dev(case.dev.data_ptr(), case.dev.data_ptr(), 1, 0, 1e-2, out4, eng._stream()) == -1
    assert eng.rel_check(case.dev, case.dev, 0.0) == (0.0, 0, 0, int((~case.zero).sum()))
    for eps, isf in ((1e-2, True), (1e-2, False), (R.tolerance_floor(True), True), (R.tolerance_floor(False), False)):
        assert eng.rel_tolerance(eps, isf) == R.tolerance(eps, isf)


def test_a_pair_behind_pending_work_on_a_side_stream(eng):
    """the source is still being produced on a non-default stream when compress_rel is queued there, and the decode is
    queued behind the compress"""
    import torch
    case = _cases.get("vort_chunks") or Case(eng, "vort_chunks")
    st = torch.cuda.Stream()
    host = torch.from_numpy(case.vol).pin_memory()
    with torch.cuda.stream(st):
        big = torch.ones(2048, 2048, device="cuda")
        for _ in range(20):   # work the stream has to get through first
            big = (big @ big) * (1.0 / 2048.0)
        src = torch.empty(case.vol.shape, dtype=torch.float32, device="cuda")
        src.copy_(host, non_blocking=True)
        src = src * 1.0   # (a kernel between the copy and the call; it keeps the sign of -0.0)
        container, side = eng.compress_rel(src, case.chunks, case.eps)
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
container, side = eng.compress_rel(vol, (20, 18, 16), 1e-2)
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
    """SPERR_HIP_POISON=0xFF for a whole child process: the engine's buffers -- relStage and relWork among them -- are
    filled with NaNs before every call carves them, behind a fixed-rate call of another chunk shape"""
    import os
    import subprocess
    import sys
    case = _cases.get("vort_chunks") or Case(eng, "vort_chunks")
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
