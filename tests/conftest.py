import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def _ref_session():
    """(the real reference build oracle/_ref or None where it is not built, the recorded digests, recording?)"""
    import refbits
    from oracle import pyoracle
    recording = bool(os.environ.get(refbits.RECORD_ENV))
    live = pyoracle.Ref() if pyoracle.have_ref() else None
    if recording and live is None:
        pytest.exit("recording the reference's digests needs oracle/_ref")
    table = refbits.load_table(recording)
    yield live, table, recording
    if recording:
        refbits.save_table(table)


@pytest.fixture
def ref(request, _ref_session):
    """The reference's results for this test (tests/refbits.py): from the real reference build
    (oracle/_ref) where it is present, else the digests recorded from it."""
    import refbits
    return refbits.RefBits(request.node.nodeid.split("::", 1)[1], *_ref_session)
