"""GPU: the device calls as an application makes them -- behind work that is still pending on the caller's stream, and
from more host threads than a device has engines (include/sperr_hip.h, DESIGN.md section 1 "Engines").

Every expected byte and value comes from the oracle (oracle/pyoracle.py), tests/mask_model.py or the numpy model of
the quality figures (tests/quality_cases.py), computed on the CPU from the TRUE inputs.  Containers and masks are
compared byte for byte, values bit for bit through integer views, quality figures as tests/test_gpu_quality.py does.

A. pending inputs (test_call_behind_pending_inputs, one case per front of FRONTS).  Every device input buffer first
   holds a DECOY: another finite field of the same shape and dtype, or another valid container / stream / mask of the
   same volume shape, chunking, mode and dtype, in the same buffer (the call gets a view of the true input's length).
   A decoy container of a single-container front is coded at another bit rate, so that its header differs from the
   true one's in the chunk lengths: a decode that parses the decoy's header refuses the true container's length.
   After torch.cuda.synchronize() a fresh stream s gets a delay (torch.cuda._sleep, calibrated with two events), the
   copies of the true inputs over the decoys and an event; `not event.query()` is the witness that the call is entered
   with its inputs unwritten.  The call is made at once; its outputs are cloned on s with no synchronisation of any
   kind, and on a second stream that waits for an event of s.  A call that reads an input ahead of s's order -- a
   side stream that does not wait for the fork event, a header read on the default stream -- computes from the decoy:
   a well-formed, different result, or a refusal; never a fault.
   test_call_beside_a_busy_default_stream runs the same fronts with the delay on the DEFAULT stream instead and only
   the clone on s: a kernel that a call leaves on the default stream sits behind that delay, and the clone misses
   it.  (sperrhip_mask_apply_dev and sperrhip_mask_expand_dev read their mask's header on the caller's stream and
   wait for it, so by the time their kernel is enqueued nothing is pending on s any more: the first test alone
   cannot tell where that kernel went.)
   Streams share hardware queues (four per process by default, handed out in turn), and work on the default stream
   that lands in the queue of s runs behind s's delay as if it had waited for it -- on an MI355X a header read on
   the default stream went unseen at every second front.  So each delayed run is made twice, the two streams
   changing roles: streams created one after the other lie in different queues, and at most one of them in the
   default stream's.
   The delay: a module fixture runs every front warmed and undelayed five times, takes the median wall time of each
   and sets the delay to four times the slowest, at least 20 ms.  Measured on an MI355X: see DELAY NOTES below.
   Shapes are the issue's.  Substitutions, each on the same path:
     * boxes "not sharing chunks": two entries of 24^3 of ONE container of (48, 48, 48) in 16^3 always share a chunk
       (the boxes [0, 24) and [24, 48) both meet chunk 1 of every axis), so that case takes three container tensors,
       one entry each, where the other takes two containers and entries (0, 0, 1); boxes_plan() says which is staged.
     * the level: chunks of 16^3 have one coarser level, level 0 (32^3 for the volume), so row 2's container is
       decoded at level 0, not 1.
     * parse_header gets a case of its own with a decoy of ANOTHER volume shape: the decoy the scheme prescribes has
       the true container's dims, chunking and dtype, so its header parses to the same values and a stale read of it
       cannot show in what parse_header or a decode that sizes its output from it returns.  mask_parse can tell
       (nmissing differs between two balls).

B. more callers than engines (test_six_threads_*, test_small_pools_*, test_release_during_calls): threads behind a
   Barrier, one SperrHip, a torch stream per thread, failures collected in a list, every join with a time limit.

DELAY NOTES (MI355X, three runs of the module): the slowest warmed fronts are decompress_r1 and
decompress_strided_out_r1 at 9.2 to 9.7 ms (median of 5, wall); the decodes of the other containers take 3.5 to 8 ms,
the compressions 0.8 to 2.6 ms, quality, truncate and the mask calls 0.03 to 0.5 ms.  The delay came to 37.0, 37.0 and
38.8 ms (2.39 million cycles of torch.cuda._sleep per ms; the fixture measures the sleep it will use and prints every
front's time with pytest -s).  The module runs in 15 s.
"""
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np
import pytest

import mask_model as M
import quality_cases as qc
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = {4: 0x7FC0BEEF, 8: 0x7FF80000DEADBEEF}
BITWISE = ("mse", "rmse", "linfty", "mean", "var")      # (tests/test_gpu_quality.py)
JOIN_SECONDS = 120


# ---- comparing ---------------------------------------------------------------------------------------------------
def u8(b):
    return np.frombuffer(b, dtype=np.uint8).copy()


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Figures:
    """the quality figures of (a, b) by the numpy model, compared as tests/test_gpu_quality.py::check compares them"""

    def __init__(self, a, b):
        self.dt = a.dtype.type
        self.want = qc.model(np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1))

    def differs(self, q):
        dt = self.dt
        for f in BITWISE:
            if qc.to_hex(dt(getattr(q, f))) != qc.to_hex(dt(self.want[f])):
                return f"{f}: {getattr(q, f)!r} for {self.want[f]!r}"
        for f in ("min", "max"):
            if dt(getattr(q, f)) != dt(self.want[f]):
                return f"{f}: {getattr(q, f)!r} for {self.want[f]!r}"
        if qc.ulp_distance(dt(q.psnr), dt(self.want["psnr"]), dt) > 8:
            return f"psnr: {q.psnr!r} for {self.want['psnr']!r}"
        return None


def differs(got, want):
    """None when `got` is `want`, else a word about the first difference.  got: a cuda tensor, a Quality, a host
    value, or a list of such; want: a numpy array (bytes / bits / bools), a Figures, a host value (a tuple: of ints),
    or a list of such"""
    if isinstance(want, list):
        if not isinstance(got, (list, tuple)) or len(got) != len(want):
            return f"{type(got).__name__} of {len(got) if hasattr(got, '__len__') else '?'} for {len(want)} results"
        for i, (g, w) in enumerate(zip(got, want)):
            d = differs(g, w)
            if d:
                return f"[{i}] {d}"
        return None
    if isinstance(want, Figures):
        return want.differs(got)
    if isinstance(want, np.ndarray):
        g = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
        if g.shape != want.shape or g.dtype != want.dtype:
            return f"{g.dtype}{g.shape} for {want.dtype}{want.shape}"
        if want.dtype == bool:
            bad = np.flatnonzero(g.reshape(-1) != want.reshape(-1))
        else:
            bad = np.flatnonzero(ibits(g).reshape(-1) != ibits(want).reshape(-1))
        return None if bad.size == 0 else f"{bad.size} of {want.size} elements differ, the first at {int(bad[0])}"
    if isinstance(want, tuple):
        want = tuple(int(v) for v in want)
        got = tuple(int(v) for v in got)
    return None if got == want else f"{got!r} for {want!r}"


# ---- a front: its pending inputs, the call, what the oracle says -------------------------------------------------
class In:
    """one device input: `true` and `decoy` are numpy arrays of one dtype; a container, stream or mask (uint8, 1-D)
    may differ from its decoy in length, anything else has its decoy's shape"""

    def __init__(self, true, decoy):
        self.true, self.decoy = np.ascontiguousarray(true), np.ascontiguousarray(decoy)
        assert self.true.dtype == self.decoy.dtype
        if self.true.dtype == np.uint8 and self.true.ndim == 1:
            assert self.true.tobytes() != self.decoy.tobytes()
        else:
            assert self.true.shape == self.decoy.shape and np.isfinite(self.decoy).all()
            assert not np.array_equal(ibits(self.true), ibits(self.decoy))

    def stage(self):
        import torch
        self.d_true = torch.from_numpy(self.true.reshape(-1)).cuda()
        self.d_decoy = torch.from_numpy(self.decoy.reshape(-1)).cuda()
        self.buf = torch.zeros(max(self.true.size, self.decoy.size), dtype=self.d_true.dtype, device="cuda")

    def arm(self):
        self.buf[:self.decoy.size].copy_(self.d_decoy)

    def fire(self):
        self.buf[:self.true.size].copy_(self.d_true, non_blocking=True)

    def view(self):
        return self.buf[:self.true.size].view(self.true.shape)


class Front:
    """inputs: the In's; call(eng, *views) -> the results (cuda tensors, Quality records, host values, lists of
    them); want: what they must be, in the same layout"""

    def __init__(self, inputs, call, want):
        self.inputs, self.call, self.want = inputs, call, want
        self.staged = False

    def stage(self):
        if not self.staged:
            for i in self.inputs:
                i.stage()
            self.staged = True


def field(shape, seed, dtype=np.float32):
    return turbulence(shape, seed=seed, dtype=dtype)


def noisy(shape, seed, dtype=np.float32):
    """tests/test_gpu_fuzz.py::make_case, kind 2: many outliers in PWE mode, several bit planes of them"""
    rng = np.random.default_rng(seed)
    return (turbulence(shape, seed=seed + 5, dtype=np.float64) +
            0.2 * rng.standard_normal(shape) * (rng.random(shape) < 0.2)).astype(dtype)


def crop(a, lo_xyz, dims_xyz):
    (x, y, z), (dx, dy, dz) = lo_xyz, dims_xyz
    return np.ascontiguousarray(a[z:z + dz, y:y + dy, x:x + dx])


def chunk_shapes(oracle, container):
    """(number of chunks, number of distinct chunk shapes) from a container's own header: volume dims at bytes 2..13,
    chunk dims at 14..19 when the flag byte says the volume has more than one chunk (SPERR3D_OMP_C.cpp:170-210)"""
    vol = [int(v) for v in np.frombuffer(container[2:14], dtype="<u4")]
    ch = [int(v) for v in np.frombuffer(container[14:20], dtype="<u2")] if container[1] & 0x10 else vol
    cells = oracle.chunk_volume(vol, ch)
    return len(cells), len({(int(c[1]), int(c[3]), int(c[5])) for c in cells})


class Bank:
    """the fields, their decoys and the oracle's containers, made once (the oracle is the slow part)"""

    def __init__(self, oracle):
        self.o = oracle
        self.memo = {}

    def get(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    # (name -> (true field, decoy field, chunks, mode, quality))
    def row(self, name):
        def make():
            if name == "r1":
                return field((50, 64, 72), 1), field((50, 64, 72), 101), (32, 32, 32), 1, 2.0
            if name == "r2":
                return field((64, 64, 64), 2), field((64, 64, 64), 102), (16, 16, 16), 1, 4.0
            if name == "r3":
                return (field((64, 64, 64), 3, np.float64), field((64, 64, 64), 103, np.float64), (64, 64, 64), 2,
                        90.0)
            if name == "r4":
                return noisy((48, 32, 48), 4), noisy((48, 32, 48), 104), (16, 16, 24), 3, 1e-3
            if name == "box":       # the containers of the boxes call
                return field((48, 48, 48), 5), field((48, 48, 48), 105), (16, 16, 16), 1, 3.0
            if name == "box2":
                return field((48, 48, 48), 6), field((48, 48, 48), 106), (16, 16, 16), 1, 3.0
            raise KeyError(name)
        return self.get(("row", name), make)

    def cont(self, name, decoy=False):
        v, d, ch, mode, q = self.row(name)
        # (a decoy container is coded at three quarters of the rate: its chunk lengths, and so its header, differ)
        dq = 0.75 * q if mode == 1 else q
        return self.get(("cont", name, decoy), lambda: self.o.comp_3d(d if decoy else v, ch, mode, dq if decoy else q))

    def cont_in(self, name):
        return In(u8(self.cont(name)), u8(self.cont(name, True)))

    def decoded(self, name, as_float=True):
        return self.get(("dec", name, as_float), lambda: self.o.decomp_3d(self.cont(name), as_float))

    def batch(self):
        def make():
            vols = [np.stack([field((24, 28, 40), 90 + 10 * k + s, np.float64) for s in range(4)]) for k in (0, 1)]
            conts = [[self.o.comp_3d(v, (16, 16, 16), 1, 3.0) for v in vs] for vs in vols]
            assert [len(c) for c in conts[0]] == [len(c) for c in conts[1]], "the decoy batch must lie as the true one"
            return vols, conts
        return self.get("batch", make)

    def slices(self):
        def make():
            one = [field((1, 96, 121), 20 + k)[0] for k in (0, 1)]
            four = [np.stack([field((1, 28, 40), 30 + 10 * k + s)[0] for s in range(4)]) for k in (0, 1)]
            s1 = [self.o.comp_2d(im, 1, 2.0, False) for im in one]
            s4 = [[self.o.comp_2d(im, 1, 2.0, False) for im in st] for st in four]
            assert [len(c) for c in s4[0]] == [len(c) for c in s4[1]], "the decoy batch must lie as the true one"
            return one, four, s1, s4
        return self.get("slices", make)

    def fields(self):
        def make():
            # (z, y, x, c): turbulence, the same a hundred times as large, another turbulence
            arrs = []
            for k in (0, 1):
                a = field((16, 24, 40), 40 + k)
                arrs.append(np.ascontiguousarray(np.stack([a, 100.0 * a, field((16, 24, 40), 50 + k)], axis=-1)))
            conts = [[self.o.comp_3d(np.ascontiguousarray(a[..., f]), (16, 16, 16), 1, 3.0) for f in range(3)]
                     for a in arrs]
            assert [len(c) for c in conts[0]] == [len(c) for c in conts[1]], "the decoy fields must lie as the true ones"
            back = [np.ascontiguousarray(np.stack([self.o.decomp_3d(c, True) for c in cs], axis=-1)) for cs in conts]
            return arrs, conts, back
        return self.get("fields", make)

    def masked(self):
        def make():
            shape = (40, 48, 56)
            out = []
            for k, radius in ((0, 12), (1, 9)):
                miss = M.ball_mask(shape, radius)
                v = field(shape, 60 + k)
                v[miss] = np.nan
                filled = M.filled(v, miss)
                cont = self.o.comp_3d(filled, (32, 32, 32), 1, 2.0 - 0.5 * k)
                out.append(dict(vol=v, miss=miss, filled=filled, stream=M.stream(miss), cont=cont,
                                back=self.o.decomp_3d(cont, True)))
            return out
        return self.get("masked", make)


def sentinel_like(shape, dtype):
    import torch
    esz = np.dtype(dtype).itemsize
    p = torch.full(tuple(shape), SENTINEL[esz], dtype=torch.int32 if esz == 4 else torch.int64, device="cuda")
    return p.view(torch.float32 if esz == 4 else torch.float64)


def sentinel_host(shape, dtype):
    esz = np.dtype(dtype).itemsize
    return np.full(shape, SENTINEL[esz], dtype=np.uint32 if esz == 4 else np.uint64).view(dtype)


def lay(conts):
    """containers back to back: (bytes, offsets)"""
    offs = np.concatenate([[0], np.cumsum([len(c) for c in conts])]).astype(int)
    return u8(b"".join(conts)), offs


def split(buf, offs):
    return [buf[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def make_front(name, bank):
    """the front `name` of FRONTS"""
    o = bank.o
    if name in ("compress_r1", "compress_r2", "compress_r3_psnr_f64", "compress_r4_pwe"):
        row = name.split("_")[1]
        v, d, ch, mode, q = bank.row(row)
        if row == "r1":
            assert chunk_shapes(o, bank.cont(row))[1] > 1, "row 1 needs more than one chunk shape"
        if row == "r2":
            assert chunk_shapes(o, bank.cont(row)) == (64, 1), "row 2 needs 64 chunks of one shape"
        return Front([In(v, d)], lambda e, x: e.compress(x, ch, q, mode=mode), u8(bank.cont(row)))
    if name == "compress_view":
        v, d = field((40, 44, 52), 7), field((40, 44, 52), 107)
        want = o.comp_3d(np.ascontiguousarray(v[4:-4, 4:-4, 4:-4]), (32, 32, 32), 1, 2.0)
        return Front([In(v, d)], lambda e, x: e.compress(x[4:-4, 4:-4, 4:-4], (32, 32, 32), 2.0), u8(want))
    if name in ("decompress_r1", "decompress_r2", "decompress_r4", "decompress_r4_f64"):
        row = name.split("_")[1]
        of = not name.endswith("_f64")
        if row == "r2":
            assert chunk_shapes(o, bank.cont(row)) == (64, 1), "row 6 needs the 64 chunks of row 2"
        shape = bank.row(row)[0].shape
        return Front([bank.cont_in(row)], lambda e, c: e.decompress(c, output_float=of, shape_zyx=shape),
                     bank.decoded(row, of))
    if name == "decompress_header_r2":
        return Front([bank.cont_in("r2")], lambda e, c: e.decompress(c), bank.decoded("r2"))
    if name == "parse_header":
        other = o.comp_3d(field((40, 48, 56), 8), (32, 32, 32), 1, 2.0)
        return Front([In(u8(bank.cont("r2")), u8(other))], lambda e, c: list(e.parse_header(c)),
                     [(64, 64, 64), True, (16, 16, 16)])
    if name == "decompress_box_r2":
        lo, dims = (8, 8, 8), (24, 24, 24)
        return Front([bank.cont_in("r2")], lambda e, c: e.decompress_box(c, lo, dims),
                     crop(bank.decoded("r2"), lo, dims))
    if name == "decompress_level_r2":
        levels = o.decomp_3d_multi_res(bank.cont("r2"))[1]
        assert len(levels) == 1 and levels[0].shape == (32, 32, 32)
        # (no box and no `out`: the wrapper sizes the level from the header)
        return Front([bank.cont_in("r2")], lambda e, c: e.decompress_level(c, 0), levels[0])
    if name == "decompress_pct40_r2":
        want = o.decomp_3d(o.trunc_3d(bank.cont("r2"), 40), True)
        return Front([bank.cont_in("r2")], lambda e, c: e.decompress(c, pct=40), want)
    if name == "decompress_strided_out_r1":
        dec = bank.decoded("r1")
        dz, dy, dx = dec.shape
        want = sentinel_host((dz + 4, dy + 6, dx + 10), np.float32)
        want[2:-2, 3:-3, 5:-5] = dec

        def call(e, c):
            parent = sentinel_like((dz + 4, dy + 6, dx + 10), np.float32)
            e.decompress(c, out=parent[2:-2, 3:-3, 5:-5], shape_zyx=dec.shape)
            return parent
        return Front([bank.cont_in("r1")], call, want)
    if name == "compress_batch_f64":
        vols, conts = bank.batch()
        return Front([In(vols[0], vols[1])], lambda e, x: e.compress_batch(x, (16, 16, 16), 3.0),
                     [u8(c) for c in conts[0]])
    if name == "decompress_batch_f64":
        vols, conts = bank.batch()
        (t, offs), (d, _) = lay(conts[0]), lay(conts[1])
        want = np.stack([o.decomp_3d(c, False) for c in conts[0]])
        return Front([In(t, d)], lambda e, c: e.decompress_batch(split(c, offs), output_float=False), want)
    if name in ("compress_2d", "decompress_2d", "compress_2d_batch", "decompress_2d_batch"):
        one, four, s1, s4 = bank.slices()
        if name == "compress_2d":
            return Front([In(one[0], one[1])], lambda e, x: e.compress_2d(x, 2.0), u8(s1[0]))
        if name == "decompress_2d":
            return Front([In(u8(s1[0]), u8(s1[1]))], lambda e, c: e.decompress_2d(c, (96, 121)),
                         o.decomp_2d(s1[0], (96, 121), True))
        if name == "compress_2d_batch":
            return Front([In(four[0], four[1])], lambda e, x: e.compress_2d_batch(x, 2.0), [u8(c) for c in s4[0]])
        (t, offs), (d, _) = lay(s4[0]), lay(s4[1])
        want = np.stack([o.decomp_2d(c, (28, 40), True) for c in s4[0]])
        return Front([In(t, d)], lambda e, c: e.decompress_2d_batch(split(c, offs), (28, 40)), want)
    if name in ("compress_fields", "decompress_fields", "quality_fields"):
        arrs, conts, back = bank.fields()
        if name == "compress_fields":
            return Front([In(arrs[0], arrs[1])], lambda e, x: e.compress_fields(x, (16, 16, 16), 3.0),
                         [u8(c) for c in conts[0]])
        if name == "decompress_fields":
            (t, offs), (d, _) = lay(conts[0]), lay(conts[1])
            return Front([In(t, d)], lambda e, c: e.decompress_fields(split(c, offs)), back[0])
        want = [Figures(arrs[0][..., f], back[0][..., f]) for f in range(3)]
        return Front([In(arrs[0], arrs[1]), In(back[0], back[1])], lambda e, a, b: e.quality_fields(a, b), want)
    if name in ("decompress_boxes_shared", "decompress_boxes_apart"):
        dims = (24, 24, 24)
        decs = [bank.decoded("box"), bank.decoded("box2")]
        if name == "decompress_boxes_shared":
            which, los = [0, 0, 1], [(0, 0, 0), (8, 8, 8), (24, 16, 8)]
            ins = [bank.cont_in("box"), bank.cont_in("box2")]
            call = lambda e, a, b: [e.boxes_plan((48, 48, 48), [(16, 16, 16)] * 2, los, dims, which)["staged"],
                                    e.decompress_boxes([a, b], los, dims, which)]
            staged = True
        else:
            which, los = [0, 1, 0], [(0, 0, 0), (24, 24, 24), (24, 8, 16)]
            ins = [bank.cont_in("box"), bank.cont_in("box2"), bank.cont_in("box")]
            call = lambda e, a, b, c: [e.boxes_plan((48, 48, 48), [(16, 16, 16)] * 3, los, dims)["staged"],
                                       e.decompress_boxes([a, b, c], los, dims)]
            staged = False
        want = np.stack([crop(decs[w], lo, dims) for w, lo in zip(which, los)])
        return Front(ins, call, [staged, want])
    if name == "truncate_r2":
        return Front([bank.cont_in("r2")], lambda e, c: e.truncate(c, 25), u8(o.trunc_3d(bank.cont("r2"), 25)))
    if name == "quality":
        v, d = bank.row("r1")[:2]
        back = bank.decoded("r1")
        other = o.decomp_3d(bank.cont("r1", True), True)
        return Front([In(v, d), In(back, other)], lambda e, a, b: e.quality(a, b), Figures(v, back))
    mk = bank.masked()
    t, d = mk[0], mk[1]
    finite_decoy = d["filled"]                 # (a decoy volume is finite: the decoy's in-filled field)
    if name == "mask_make":
        def call(e, x):
            import torch
            filled = torch.empty_like(x)
            stream, nmiss = e.mask_make(x, "nan", filled_out=filled)
            return [stream, nmiss, filled]
        return Front([In(t["vol"], finite_decoy)], call, [u8(t["stream"]), int(t["miss"].sum()), t["filled"]])
    if name == "mask_apply":
        want = t["filled"].copy()
        want[t["miss"]] = np.float32(1e20)
        return Front([In(t["filled"], finite_decoy), In(u8(t["stream"]), u8(d["stream"]))],
                     lambda e, x, m: e.mask_apply(x, m, 1e20), want)
    if name == "mask_expand":
        return Front([In(u8(t["stream"]), u8(d["stream"]))], lambda e, m: e.mask_bits(m), t["miss"].reshape(-1))
    if name == "mask_parse":
        return Front([In(u8(t["stream"]), u8(d["stream"]))], lambda e, m: [e.mask_parse(m)],
                     [(t["miss"].size, int(t["miss"].sum()), M.parse(t["stream"])[0])])
    if name == "compress_masked":
        return Front([In(t["vol"], finite_decoy)], lambda e, x: list(e.compress_masked(x, (32, 32, 32), 2.0)),
                     [u8(t["cont"]), u8(t["stream"])])
    if name == "decompress_masked":
        want = t["back"].copy()
        want[t["miss"]] = np.float32(np.nan)
        return Front([In(u8(t["cont"]), u8(d["cont"])), In(u8(t["stream"]), u8(d["stream"]))],
                     lambda e, c, m: e.decompress_masked(c, m), want)
    if name == "quality_masked":
        keep = ~t["miss"]
        return Front([In(t["vol"], finite_decoy), In(t["back"], d["back"]), In(u8(t["stream"]), u8(d["stream"]))],
                     lambda e, a, b, m: e.quality_masked(a, b, m), Figures(t["vol"][keep], t["back"][keep]))
    raise KeyError(name)


FRONTS = ["compress_r1", "compress_r2", "compress_r3_psnr_f64", "compress_r4_pwe", "compress_view",
          "decompress_r1", "decompress_r2", "decompress_r4", "decompress_r4_f64", "decompress_header_r2", "parse_header",
          "decompress_box_r2", "decompress_level_r2", "decompress_pct40_r2", "decompress_strided_out_r1",
          "compress_batch_f64", "decompress_batch_f64",
          "compress_2d", "decompress_2d", "compress_2d_batch", "decompress_2d_batch",
          "compress_fields", "decompress_fields", "quality_fields",
          "decompress_boxes_shared", "decompress_boxes_apart", "truncate_r2", "quality",
          "mask_make", "mask_apply", "mask_expand", "mask_parse", "compress_masked", "decompress_masked",
          "quality_masked"]


# ---- fixtures ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    yield e
    e.release()


@pytest.fixture(scope="module")
def bank(oracle):
    return Bank(oracle)


@pytest.fixture(scope="module")
def fronts(bank):
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = make_front(name, bank)
            memo[name].stage()
        return memo[name]
    return get


def results(out):
    """the results of a call as a list (a lone result: a list of one)"""
    return out if isinstance(out, list) else [out]


def clone_all(out):
    return [clone_all(r) if isinstance(r, list) else (r.clone() if hasattr(r, "clone") else r) for r in out]


def run_front(eng, front, sleep_cycles=0, busy_default=False):
    """steps 1 to 7 of the module docstring, twice when there is a delay: the two streams change roles.  Returns the
    words about what differs (none: all is well)"""
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    said = run_once(eng, front, a, b, sleep_cycles, busy_default)
    if sleep_cycles and not said:
        said = run_once(eng, front, b, a, sleep_cycles, busy_default)
    return said


def run_once(eng, front, s, s2, sleep_cycles, busy_default):
    import torch
    for i in front.inputs:
        i.arm()
    torch.cuda.synchronize()
    witness = torch.cuda.Event()
    if busy_default and sleep_cycles:
        torch.cuda._sleep(sleep_cycles)
        witness.record()
    with torch.cuda.stream(s):
        if sleep_cycles and not busy_default:
            torch.cuda._sleep(sleep_cycles)
        for i in front.inputs:
            i.fire()
        if not busy_default:
            witness.record(s)
        if sleep_cycles:
            assert not witness.query(), "the delay was over before the call was made: nothing was pending"
        out = results(front.call(eng, *[i.view() for i in front.inputs]))
        on_s = clone_all(out)
        done = torch.cuda.Event()
        done.record(s)
    with torch.cuda.stream(s2):
        s2.wait_event(done)
        on_s2 = clone_all(out)
    s.synchronize()
    s2.synchronize()
    said = []
    for what, got in (("the call's own result", out), ("its clone on the caller's stream", on_s),
                      ("its clone on a stream that waited for the caller's", on_s2)):
        d = differs(got, results(front.want))
        if d:
            said.append(f"{what}: {d}")
    torch.cuda.synchronize()
    return said


@pytest.fixture(scope="module")
def delay(eng, fronts):
    """(cycles for torch.cuda._sleep, the delay in ms): four times the slowest warmed front, at least 20 ms"""
    import torch
    torch.cuda._sleep(1000)                                  # (the sleep kernel's own first launch)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 20 * 1000 * 1000
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    torch.cuda.synchronize()
    per_ms = probe / a.elapsed_time(b)
    slowest = 0.0
    for name in FRONTS:
        f = fronts(name)
        assert run_front(eng, f) == [], name                 # the warming run: undelayed, and right
        times = []
        for _ in range(5):
            for i in f.inputs:
                i.fire()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f.call(eng, *[i.view() for i in f.inputs])
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        med = sorted(times)[2]
        print(f"front {name}: {med:.2f} ms")
        slowest = max(slowest, med)
    ms = max(20.0, 4.0 * slowest)
    cycles = int(ms * per_ms)
    # the sleep is what it was calibrated to be
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    torch.cuda.synchronize()
    took = a.elapsed_time(b)
    print(f"slowest front {slowest:.2f} ms; delay {ms:.1f} ms = {cycles} cycles ({per_ms:.0f} per ms), measured {took:.1f} ms")
    assert took >= 0.9 * ms, (took, ms)
    return cycles, ms


# ---- A ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FRONTS)
def test_call_behind_pending_inputs(eng, fronts, delay, name):
    said = run_front(eng, fronts(name), sleep_cycles=delay[0])
    assert said == [], (name, said)


@pytest.mark.parametrize("name", FRONTS)
def test_call_beside_a_busy_default_stream(eng, fronts, delay, name):
    said = run_front(eng, fronts(name), sleep_cycles=delay[0], busy_default=True)
    assert said == [], (name, said)


# ---- B ------------------------------------------------------------------------------------------------------------
MIXES = ["r1", "r4", "batch", "fields", "boxes", "masked"]


def mix_data(bank, mix):
    """the host inputs and expected results of a thread's front mix, as a dict of numpy arrays (they travel to the
    child processes as .npy files)"""
    o = bank.o
    if mix in ("r1", "r4"):
        v = bank.row(mix)[0]
        return dict(vol=v, cont=u8(bank.cont(mix)), dec=bank.decoded(mix))
    if mix == "batch":
        vols, conts = bank.batch()
        t, offs = lay(conts[0])
        return dict(vol=vols[0], cont=t, offs=offs, dec=np.stack([o.decomp_3d(c, False) for c in conts[0]]))
    if mix == "fields":
        arrs, conts, back = bank.fields()
        t, offs = lay(conts[0])
        return dict(vol=arrs[0], cont=t, offs=offs, dec=back[0])
    if mix == "boxes":
        f = make_front("decompress_boxes_shared", bank)
        return dict(a=f.inputs[0].true, b=f.inputs[1].true, dec=f.want[1])
    mk = bank.masked()[0]
    want = mk["back"].copy()
    want[mk["miss"]] = np.float32(np.nan)
    return dict(vol=mk["vol"], cont=u8(mk["cont"]), mask=u8(mk["stream"]), dec=want)


MIX_SETTINGS = {"r1": ((32, 32, 32), 1, 2.0), "r4": ((16, 16, 24), 3, 1e-3)}


def run_mix(eng, name, d):
    """one round of a mix ("kind", or "kind#label" for a second thread on the same kind) on the current stream: the
    words about what differs"""
    import torch
    mix = name.split("#")[0]
    cu = lambda a: torch.from_numpy(a).cuda()
    said = []

    def check(what, got, want):
        w = differs(got, want)
        if w:
            said.append(f"{mix} {what}: {w}")
    if mix in MIX_SETTINGS:
        ch, mode, q = MIX_SETTINGS[mix]
        c = eng.compress(cu(d["vol"]), ch, q, mode=mode)
        check("compress", c, d["cont"])
        check("decompress", eng.decompress(cu(d["cont"])), d["dec"])
    elif mix == "batch":
        offs = [int(v) for v in d["offs"]]
        parts = eng.compress_batch(cu(d["vol"]), (16, 16, 16), 3.0)
        check("compress_batch", torch.cat(parts), d["cont"])
        check("decompress_batch", eng.decompress_batch(split(cu(d["cont"]), offs), output_float=False), d["dec"])
    elif mix == "fields":
        offs = [int(v) for v in d["offs"]]
        parts = eng.compress_fields(cu(d["vol"]), (16, 16, 16), 3.0)
        check("compress_fields", torch.cat(parts), d["cont"])
        check("decompress_fields", eng.decompress_fields(split(cu(d["cont"]), offs)), d["dec"])
    elif mix == "boxes":
        got = eng.decompress_boxes([cu(d["a"]), cu(d["b"])], [(0, 0, 0), (8, 8, 8), (24, 16, 8)], (24, 24, 24), [0, 0, 1])
        check("decompress_boxes", got, d["dec"])
    else:
        c, m = eng.compress_masked(cu(d["vol"]), (32, 32, 32), 2.0)
        check("compress_masked container", c, d["cont"])
        check("compress_masked mask", m, d["mask"])
        check("decompress_masked", eng.decompress_masked(cu(d["cont"]), cu(d["mask"])), d["dec"])
    torch.cuda.current_stream().synchronize()
    return said


def run_threads(eng, data, mixes, rounds, extra=None):
    """a thread per mix behind a barrier, each under a stream of its own; `extra`: one more thread's function.
    Returns (failures, threads that did not come back in time)"""
    import torch
    bad = []
    n = len(mixes) + (1 if extra else 0)
    gate = threading.Barrier(n)

    def work(mix):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                gate.wait(JOIN_SECONDS)
                for r in range(rounds):
                    bad.extend(f"round {r}: {w}" for w in run_mix(eng, mix, data[mix]))
        except Exception as exc:   # noqa: BLE001  (a thread's exception is a failure of the test, not lost)
            bad.append(f"{mix}: {type(exc).__name__}: {exc}")

    def other():
        try:
            gate.wait(JOIN_SECONDS)
            extra()
        except Exception as exc:   # noqa: BLE001
            bad.append(f"extra: {type(exc).__name__}: {exc}")
    ts = [threading.Thread(target=work, args=(m,), daemon=True) for m in mixes]
    if extra:
        ts.append(threading.Thread(target=other, daemon=True))
    for t in ts:
        t.start()
    stuck = []
    deadline = time.monotonic() + JOIN_SECONDS
    for t in ts:
        t.join(max(0.0, deadline - time.monotonic()))
        if t.is_alive():
            stuck.append(t.name)
    return bad, stuck


@pytest.fixture(scope="module")
def mixes(bank):
    return {m: mix_data(bank, m) for m in MIXES}


def test_six_threads_three_rounds_of_mixed_fronts(eng, mixes):
    """six callers for the pool's four engines: two wait on the host each round, and an engine goes from a front to
    one that owns other buffers"""
    for m in MIXES:                                             # (warm, one thread: plans and buffers)
        assert run_mix(eng, m, mixes[m]) == [], m
    bad, stuck = run_threads(eng, mixes, MIXES, rounds=3)
    assert not stuck, f"threads that did not return within {JOIN_SECONDS} s: {stuck}"
    assert not bad, bad


_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
td, names = sys.argv[2], sys.argv[3:]
import test_gpu_callers as T
from sperr_amd.api import SperrHip
eng = SperrHip()
data = {m: dict(np.load(os.path.join(td, m + ".npz"))) for m in names}
bad, stuck = T.run_threads(eng, data, names, rounds=2)
with open(os.path.join(td, "out.json"), "w") as f:
    json.dump({"bad": bad, "stuck": stuck}, f)
os._exit(1 if stuck else 0)          # (a stuck thread must not keep the process)
"""


@pytest.mark.parametrize("engines", ["1", "2"])
def test_small_pools_in_a_fresh_process(mixes, engines):
    """SPERR_HIP_ENGINES_PER_DEVICE is read once per process: a child with one engine, where every call queues
    behind the others on the host (and an entry point that held its lease across another's would never return),
    and one with two; four threads, two rounds, nothing warmed"""
    import json
    names = ["r1", "batch", "boxes", "masked"]
    with tempfile.TemporaryDirectory() as td:
        for m in names:
            np.savez(os.path.join(td, m + ".npz"), **mixes[m])
        env = dict(os.environ, SPERR_HIP_ENGINES_PER_DEVICE=engines)
        run = subprocess.run([sys.executable, "-c", _CHILD, ROOT, td] + names, env=env, timeout=300)
        with open(os.path.join(td, "out.json")) as f:
            res = json.load(f)
    assert res == {"bad": [], "stuck": []}, (engines, res)
    assert run.returncode == 0, engines


def test_release_during_calls(eng, mixes):
    """sperrhip_release() from a third thread while two compress and decode: engines in use are left alone, and one
    more release() with nothing running leaves no engine holding device memory"""
    import ctypes as C

    def releaser():
        for _ in range(10):
            eng.release()
            time.sleep(0.002)
    data = {"r1#a": mixes["r1"], "r1#b": mixes["r1"]}
    bad, stuck = run_threads(eng, data, list(data), rounds=6, extra=releaser)
    assert not stuck, f"threads that did not return within {JOIN_SECONDS} s: {stuck}"
    assert not bad, bad
    eng.release()
    eng.lib.sperrhip_debug_counter.restype = C.c_ulonglong
    eng.lib.sperrhip_debug_counter.argtypes = [C.c_int]
    assert eng.lib.sperrhip_debug_counter(6) == 0
