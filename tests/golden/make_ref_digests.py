"""Records tests/golden/ref_digests.json: the digests of what the real reference returns in
tests/test_oracle_vs_ref.py, so that those tests compare the oracle against the reference also where
oracle/_ref is not built.  Run from the repository root where it is built (oracle/Makefile `ref`):

    python tests/golden/make_ref_digests.py

It runs that test module against the live reference and rewrites the table."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import pyoracle
    if not pyoracle.have_ref():
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` first")
    os.environ["SPERR_RECORD_REF_DIGESTS"] = "1"
    sys.exit(pytest.main(["-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_vs_ref.py")]))
