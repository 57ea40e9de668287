"""What the system-taking C entry points refuse, replayed through the product library on the
device against tests/golden/capi_rules.json: the entries of capi.hip (recorded with the host-math
library), ol_trace_forbes and ol_aim_rays (recorded on the device) and, where two devices are
visible, the current-device rule.  Every buffer is a device tensor of 64 rays; the accepted calls
are a handful of 64-ray launches.  Cases, systems and buffers: tests/_capi_rules.py.
"""

from __future__ import annotations

import pytest
import torch

from optiland_amd import _capi
from tests import _capi_rules as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def context():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.zeros(1, device="cuda")
    k = R.Context(_capi.load(), R.torch_put)
    yield k
    torch.cuda.synchronize()
    k.close()


def test_every_entry_refuses_what_the_parent_refused(context):
    fix = R.fixture()
    device = dict(fix["device"])
    other = device.pop("ol_trace_ex", [])
    total = sum(len(v) for s in ("host", "device") for v in fix[s].values())
    count = R.replay(context, fix["host"], R.ENTRIES) + R.replay(context, device, R.DEVICE_ENTRIES)
    torch.cuda.synchronize()
    # (all but the two-device case below: a loader that replays nothing does not pass)
    assert count == total - len(other) and count > 0


def test_staging_refuses_what_the_parent_refused(context):
    """ol_system_create / ol_system_update through the product library: the tiny tables of
    tests/_capi_rules.py (CREATE, UPDATE), nothing but create / update / destroy calls."""
    want = R.fixture()["create"]
    got = R.create(context.lib)
    torch.cuda.synchronize()
    assert [g for g, w in zip(got, want) if g != w] == [] and len(got) == len(want) > 0


def test_current_device_rule_with_two_devices(context):
    other = R.fixture()["device"].get("ol_trace_ex")
    if torch.cuda.device_count() < 2 or not other:
        pytest.skip("needs two visible devices and the case recorded with two")
    assert [R.other_device(context)] == other
