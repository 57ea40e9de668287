"""What the C entry points of capi.hip refuse, replayed through the host-math library (an
unmodified host-only compile of capi.hip: tests/hostmath) against tests/golden/capi_rules.json --
the answers of the commit in front of the one that moved the rules into csrc/entry_rules.h.
Cases, systems and buffers: tests/_capi_rules.py.  No GPU needed.
"""

from __future__ import annotations

import pytest

from tests import _capi_rules as R
from tests import _hostmath as hm


@pytest.fixture(scope="module")
def context():
    if not hm.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    k = R.Context(hm.load(), R.numpy_put)
    yield k
    k.close()


def test_fixture_names_its_parent_and_every_entry():
    fix = R.fixture()
    assert fix["n_rays"] == R.N
    assert all(len(fix["parent"][s]) == 40 for s in ("host", "device"))
    assert sorted(fix["host"]) == sorted(R.ENTRIES)
    assert set(R.DEVICE_ENTRIES) <= set(fix["device"]) <= set(R.DEVICE_ENTRIES) | {"ol_trace_ex"}
    for section in ("host", "device"):
        for name, cases in fix[section].items():
            assert cases and all(text for _case, _rc, text in cases), name
            assert all((rc == 0) == (text == R.OK) for _case, rc, text in cases), name


def test_host_entries_refuse_what_the_parent_refused(context):
    """Code and text of every case, exactly; every peeling sequence ends with an accepted call."""
    section = R.fixture()["host"]
    assert R.replay(context, section, R.ENTRIES) == sum(len(v) for v in section.values())
