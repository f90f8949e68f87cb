"""GPU: the encoder's fused head (k_head_fused: quantiser, leaf level of the pyramid and census of the pixel passes in
one kernel, speck_enc.hip) against the three kernels it replaces.

Every case is compressed twice -- in this process with the fused head on (the default), and in a child process started
with SPERR_HIP_ENC_FUSED_HEAD=0 (the switch is read once per process) -- and both containers have to equal the CPU
oracle's byte for byte.  sperrhip_debug_counter(7) counts the batches whose 32-bit pass took the fused head: it has to
move by exactly one per shape group where the shape qualifies and the switch is on, and not at all anywhere else, so
no case can pass by quietly taking the other path.

Shapes that fuse: 256^3 (one chunk; three chunks with different data in one batch, one of them constant and one mostly
exact zeros: the histograms' -1 bins and a chunk that takes no part in the pass), 128^3 and 64^3 chunks in all three
modes, and 64^3 at rates that send chunks into the 64-bit retry behind the fused 32-bit pass.  Shapes that must not:
250^3, the border shapes of a 1000^3 volume cut into 256^3 chunks (232 along one, two and three axes), and a chunk four
samples thin."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from fields import ramp_field, smooth_field  # noqa: E402

pytestmark = pytest.mark.gpu
SWITCH = "SPERR_HIP_ENC_FUSED_HEAD"


def _three_chunks():
    """256^3 chunks side by side along x: smooth noise, a field most of whose samples are exactly zero, a constant"""
    a = smooth_field((256, 256, 256), seed=11, passes=1)
    z = smooth_field((256, 256, 256), seed=12, passes=1)
    z[np.abs(z) < np.float32(np.percentile(np.abs(z), 85))] = 0
    c = np.full((256, 256, 256), 2.5, dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([a, z, c], axis=2))


def _sparse(shape, seed):
    v = smooth_field(shape, seed=seed, passes=2)
    v[np.abs(v) < np.float32(np.percentile(np.abs(v), 60))] = 0
    return v


# name -> (field, chunk dims xyz, [(mode, quality)], batches that take the fused head per call)
CASES = {
    "one_256": (lambda: smooth_field((256, 256, 256), seed=5, passes=1), (256, 256, 256),
                [(1, 0.5), (1, 2.0), (1, 6.0)], 1),
    "three_256": (_three_chunks, (256, 256, 256), [(1, 2.0)], 1),
    "two_128": (lambda: np.concatenate([smooth_field((128, 128, 128), seed=21), _sparse((128, 128, 128), 22)], axis=0),
                (128, 128, 128), [(1, 1.0), (1, 4.0), (2, 80.0), (3, 1e-3)], 1),
    "eight_64": (lambda: smooth_field((128, 128, 128), seed=31, dtype=np.float64), (64, 64, 64),
                 [(1, 3.0), (2, 100.0), (3, 1e-4)], 1),
    "wide_retry_64": (lambda: np.concatenate([smooth_field((64, 64, 64), seed=41), ramp_field((64, 64, 64)),
                                              smooth_field((64, 64, 64), seed=42)], axis=0),
                      (64, 64, 64), [(1, 24.0), (1, 40.0)], 1),
    # a 128^3 group that fuses beside remainder groups that do not
    "mixed_groups": (lambda: smooth_field((128, 128, 224), seed=51), (128, 128, 128), [(1, 2.0)], 1),
    "not_250": (lambda: smooth_field((250, 250, 250), seed=61, passes=1), (256, 256, 256), [(1, 2.0)], 0),
    "not_border_x": (lambda: smooth_field((256, 256, 232), seed=62, passes=1), (256, 256, 256), [(1, 2.0)], 0),
    "not_border_xy": (lambda: smooth_field((256, 232, 232), seed=63, passes=1), (256, 256, 256), [(1, 2.0), (3, 1e-2)], 0),
    "not_border_xyz": (lambda: smooth_field((232, 232, 232), seed=64, passes=1), (256, 256, 256), [(1, 2.0)], 0),
    "not_thin": (lambda: smooth_field((4, 64, 64), seed=65), (64, 64, 64), [(1, 2.0), (2, 70.0)], 0),
    "not_32": (lambda: smooth_field((32, 32, 32), seed=66), (32, 32, 32), [(1, 2.0)], 0),
}


def _engine():
    import ctypes as C

    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    eng = SperrHip()
    eng.lib.sperrhip_debug_counter.restype = C.c_ulonglong
    eng.lib.sperrhip_debug_counter.argtypes = [C.c_int]
    return eng


def _compress(eng, vol, chunks, mode, q):
    """(container bytes, how far counter 7 moved)"""
    import torch
    c0 = eng.lib.sperrhip_debug_counter(7)
    out = eng.compress(torch.from_numpy(vol).cuda(), chunks, q, mode=mode)
    got = bytes(out.cpu().numpy())
    return got, int(eng.lib.sperrhip_debug_counter(7) - c0)


def _worker():
    """the child process: every case with whatever the environment says of the switch; digests and counter moves out"""
    eng = _engine()
    res = {}
    for name, (field, chunks, runs, _) in CASES.items():
        vol = field()
        for mode, q in runs:
            got, moved = _compress(eng, vol, chunks, mode, q)
            res["%s/%d/%g" % (name, mode, q)] = [hashlib.sha256(got).hexdigest(), len(got), moved]
    print("RESULT " + json.dumps(res), flush=True)


@pytest.fixture(scope="module")
def eng():
    assert os.environ.get(SWITCH, "1") != "0", "this module compares the default (fused) build path with the switch off"
    return _engine()


@pytest.fixture(scope="module")
def switched_off():
    env = dict(os.environ)
    env[SWITCH] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][len("RESULT "):])


@pytest.mark.parametrize("name", list(CASES))
def test_fused_head_parity(eng, oracle, switched_off, name):
    field, chunks, runs, batches = CASES[name]
    vol = field()
    for mode, q in runs:
        want = oracle.comp_3d(vol, chunks, mode, q)
        got, moved = _compress(eng, vol, chunks, mode, q)
        assert moved == batches, (name, mode, q, "fused batches", moved)
        assert got == want, (name, mode, q, "fused head on: container differs from the oracle's")
        digest, length, moved_off = switched_off["%s/%d/%g" % (name, mode, q)]
        assert moved_off == 0, (name, mode, q, "the switch did not take the three-kernel path")
        assert (digest, length) == (hashlib.sha256(want).hexdigest(), len(want)), (
            name, mode, q, "fused head off: container differs from the oracle's")


def test_decode_of_fused_container(eng, oracle):
    """what the fused path wrote decodes to the oracle's decode (the container is the oracle's, so this only guards the
    round trip through the library's own decoder on a fused shape)"""
    import torch
    vol = smooth_field((128, 128, 128), seed=71)
    stream = eng.compress(torch.from_numpy(vol).cuda(), (128, 128, 128), 2.0)
    back = eng.decompress(stream, output_float=True).cpu().numpy()
    ref = oracle.decomp_3d(bytes(stream.cpu().numpy()), True)
    assert np.array_equal(back.view(np.uint32), ref.view(np.uint32))


if __name__ == "__main__" and "--worker" in sys.argv:
    _worker()
