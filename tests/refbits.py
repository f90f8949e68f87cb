"""The reference's side of tests/test_oracle_vs_ref.py, with or without oracle/_ref.

Where oracle/_ref is built (the real reference, compiled by oracle/Makefile), `RefBits.get(fn)` runs
fn(pyoracle.Ref()) and returns what the reference returned.  Elsewhere it returns the SHA-256 digests of what
the reference returned for the same call of the same test, recorded in tests/golden/ref_digests.json by
tests/golden/make_ref_digests.py.  `same(ours, theirs)` compares bit for bit either way: arrays by shape, item
size and bytes (so a float array and its integer view agree), byte strings by their bytes, numbers by value,
tuples and lists element by element."""
import hashlib
import json
import os

import numpy as np
import pytest

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")
RECORD_ENV = "SPERR_RECORD_REF_DIGESTS"   # set (to any value) by make_ref_digests.py: rewrite DIGESTS


class Digest(str):
    """What the reference returned, as a digest (a value of the recorded table)."""


def digest(x):
    """x -> hex digest, or a list of them for a tuple / list (nested as x is)."""
    if isinstance(x, Digest):
        return str(x)
    if isinstance(x, (tuple, list)):
        return [digest(v) for v in x]
    h = hashlib.sha256()
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        h.update(b"nd %r %d " % (a.shape, a.itemsize))
        h.update(a.tobytes())
    elif isinstance(x, (bytes, bytearray, memoryview)):
        h.update(b"by ")
        h.update(bytes(x))
    elif isinstance(x, (bool, int, np.integer, np.bool_)):
        h.update(b"int %d" % int(x))
    elif isinstance(x, (float, np.floating)):
        h.update(b"float " + float(x).hex().encode())
    else:
        raise TypeError(f"no digest for {type(x).__name__}")
    return h.hexdigest()[:32]


def same(a, b):
    return digest(a) == digest(b)


def _replay(d):
    return tuple(_replay(v) for v in d) if isinstance(d, list) else Digest(d)


class RefBits:
    def __init__(self, test_id, live, table, recording):
        self.test_id, self.live, self.table, self.recording = test_id, live, table, recording
        self.calls = 0

    def get(self, fn):
        """fn(reference) where the reference is built, else the digests recorded for this call."""
        k = self.calls
        self.calls += 1
        recorded = self.table.get(self.test_id)
        if self.live is not None:
            got = fn(self.live)
            if self.recording:
                self.table.setdefault(self.test_id, []).append(digest(got))
            elif recorded is not None:   # the recorded digests must stay those of the reference
                assert k < len(recorded) and recorded[k] == digest(got), \
                    f"{DIGESTS} is stale for {self.test_id}: rerun tests/golden/make_ref_digests.py"
            return got
        if recorded is None or k >= len(recorded):
            pytest.fail(f"no recorded reference digests for {self.test_id} (call {k}): run "
                        "tests/golden/make_ref_digests.py where oracle/_ref is built")
        return _replay(recorded[k])


def load_table(recording):
    if recording or not os.path.exists(DIGESTS):
        return {}
    with open(DIGESTS) as f:
        return json.load(f)["digests"]


def save_table(table):
    doc = {"generator": "tests/golden/make_ref_digests.py",
           "what": "SHA-256 (first 32 hex digits) of what the reference returned, per test of "
                   "tests/test_oracle_vs_ref.py and per call of RefBits.get in it (tests/refbits.py)",
           "digests": dict(sorted(table.items()))}
    with open(DIGESTS, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
