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


def test_a_range_of_two_kinds_answers_the_kind_refused_first(context):
    """A grating row in front of a Forbes row: the range-walking entries name the Forbes row, as
    the parent did (the kinds are walked one after the other, each over the whole range), and the
    grating only where the range holds no Forbes row."""
    fix = R.fixture()
    assert len(fix["parent"]["two_kinds"]) == 40
    want = fix["two_kinds"]
    assert [c[0] for c in want] == [c[0] for c in R.TWO_KINDS]
    assert R.two_kinds(context) == want
    texts = {case: text for case, _rc, text in want}
    assert all(rc == -2 for _case, rc, _text in want)
    for case in ("ol_trace", "ol_newton_count", "ol_trace_generate"):
        assert "surface 5 is a Forbes surface" in texts[case], case
    assert "surface 3 is a diffraction grating" in texts["ol_trace in front of the forbes row"]
    assert "surface 5 is a Forbes surface" in texts["ol_trace behind the grating"]


def test_staging_refuses_what_the_parent_refused(context):
    """ol_system_create / ol_system_update, single-fault calls next to their accepted neighbours
    (tests/_capi_rules.py: CREATE, UPDATE): code and text of every case as the commit in front of
    the one that moved staging into csrc/system_stage.h answered it."""
    fix = R.fixture()
    assert len(fix["parent"]["create"]) == 40
    want = fix["create"]
    assert [(case, rc == 0) for case, rc, _text in want] == R.create_accepted()
    assert all((rc == 0) == (text == R.OK) for _case, rc, text in want)
    got = R.create(context.lib)
    assert [g for g, w in zip(got, want) if g != w] == [] and len(got) == len(want)


def test_host_entries_refuse_what_the_parent_refused(context):
    """Code and text of every case, exactly; every peeling sequence ends with an accepted call."""
    section = R.fixture()["host"]
    assert R.replay(context, section, R.ENTRIES) == sum(len(v) for v in section.values())
