import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "ref: checks against the reference (oracle/_ref/libt3ref.so, else its stored answers in tests/golden)")


@pytest.fixture(scope="session")
def orc():
    import oracle_lib
    oracle_lib.build_oracle()
    return oracle_lib.oracle()


@pytest.fixture(scope="session")
def ref(orc):
    """The unmodified reference where oracle/_ref/libt3ref.so is built (its answers checked against the stored ones), else
    its answers replayed from tests/golden/ref_calls.npz.  T3_REF_RECORD=1 rewrites that file from the live reference."""
    import oracle_lib
    if os.environ.get("T3_REF_RECORD") == "1":
        assert oracle_lib.have_ref(), "T3_REF_RECORD=1 needs oracle/_ref/libt3ref.so"
        r = oracle_lib.RecordedRef("record", orc, oracle_lib.Ref())
        yield r
        r.save()
    elif oracle_lib.have_ref():
        yield oracle_lib.RecordedRef("check", orc, oracle_lib.Ref())
    else:
        yield oracle_lib.RecordedRef("replay", orc)


@pytest.fixture(scope="session")
def t3():
    """The product's host-side mirror (ternary-image-codec_amd), loaded through __graft_entry__."""
    import __graft_entry__ as ge
    return ge.load_package()


@pytest.fixture(scope="session")
def gpu(t3):
    """Initialised device context; fails loudly (no fallback) when the HIP extension or device is missing."""
    t3.init(0)
    return t3
