"""Forbes surfaces on the MI355X (`ol_trace_forbes`, csrc/forbes.hip) against the reference's
recorded traces (tests/golden/forbes.npz, tools/make_golden_forbes.py): the one-surface launch in
fp64 and fp32 against every case, the whole singlet through `HipSystem.trace` (which splits the
range) against the fixture and against the three launches made by hand, the device against the
host run of its own source, the refusal of every range-walking entry point, status bits and the
NaN pattern.  Fixture tables only; bounds: tests/_forbes.py.

Measured on the MI355X (profiles/forbes.txt): every case within 0.03 of its bound in fp64 (tight
cases 4e-15 ... 2e-14 against 1e-12) and 0.05 in fp32 (<= 4.5e-6 against 1e-4); the whole singlet
within 1e-13 / 2.6e-5; device against the host run 9e-16; 32 tests in 2.6 s."""

import ctypes as C

import numpy as np
import pytest
import torch

from optiland_amd import _capi
from optiland_amd import system as S
from tests import _forbes as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TORCH = {np.float64: torch.float64, np.float32: torch.float32}


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from optiland_amd.engine import HipSystem
    made = {}

    def get(name):
        if name not in made:
            made[name] = HipSystem(F.case(name)["table"], DEV)
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _dev(planes, dtype=np.float64):
    return [torch.as_tensor(np.ascontiguousarray(p), dtype=TORCH[dtype], device=DEV)
            for p in planes]


def _host(planes):
    return np.stack([p.double().cpu().numpy() for p in planes])


@pytest.mark.parametrize("name", F.case_names())
def test_trace_forbes_against_every_case(name, engines):
    """All ray sets of the case in one launch (128 rays: two waves, the second nearly empty; the
    norm8 cases 1155 rays: several workgroups), the recorded row and the written-back state."""
    c = F.case(name)
    eng = engines(name)
    assert eng.can_trace_forbes() and eng.table.forbes == (F.FORBES,)
    n = c["rows"].shape[2]
    for dtype in (np.float64, np.float32):
        rays = _dev(c["rows"][F.FORBES - 1], dtype)
        row = torch.full((8, n + 5), -7.0, dtype=TORCH[dtype], device=DEV)
        status = eng.trace_forbes(rays, F.FORBES, 0, record_row=row, write_rays=True)
        assert status == 0
        got = _host(rays)
        np.testing.assert_array_equal(got, row[:, :n].double().cpu().numpy())
        assert bool((row[:, n:] == -7.0).all())          # nothing behind the n rays is written
        F.compare(got[None], c, dtype, rows=[F.FORBES], report=print)


@pytest.mark.parametrize("name", ["q_norm8_tight", "q2d_norm8_tight", "q2d_tilted_default",
                                  "q_mirror_tight", "q2d_clipped_tight"])
def test_whole_singlet_equals_fixture_and_the_three_launches(name, engines):
    c = F.case(name)
    eng = engines(name)
    n, last = c["rows"].shape[2], c["rows"].shape[0] - 1
    for dtype in (np.float64, np.float32):
        start = _dev(c["rows"][0], dtype)
        res = eng.trace(start, 0, record=True, first=0, last=last)
        assert res.status == 0
        got = res.record[:, :, :n].double().cpu().numpy()
        np.testing.assert_array_equal(_host(start), c["rows"][0].astype(dtype))   # not written
        F.compare(got, c, dtype, report=print)
        # fused run + trace_forbes + fused run, by hand, into a block of the same shape
        rec = torch.zeros_like(res.record)
        work = [t.clone() for t in start]
        eng.trace(work, 0, record=rec[:F.FORBES], first=0, last=F.FORBES - 1, write_rays=True)
        eng.trace_forbes(work, F.FORBES, 0, record_row=rec[F.FORBES], write_rays=True,
                         midrange=True)
        eng.trace(work, 0, record=rec[F.FORBES + 1:], first=F.FORBES + 1, last=last,
                  write_rays=True)
        assert torch.equal(rec[:, :, :n].view(torch.uint8), res.record[:, :, :n].view(torch.uint8))
        # ... and without a record the final state is written back into the rays
        final = [t.clone() for t in start]
        eng.trace(final, 0, record=False, first=0, last=last)
        assert torch.equal(torch.stack(final).view(torch.uint8),
                           res.record[last, :, :n].contiguous().view(torch.uint8))


def test_device_equals_the_host_run_of_its_source(engines, tmp_path):
    """fp64: 1e-13 of the plane's scale, the project's figure for device against host (the two
    differ in the hardware's division and square root only)."""
    b = F._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    exe = b.build()
    for name in ("q_norm8_tight", "q2d_norm8_tight", "q2d_mirror_tight", "q2d_flat_default"):
        c = F.case(name)
        eng = engines(name)
        rays = _dev(c["rows"][0])
        eng.trace_forbes(rays, F.FORBES, 0, write_rays=True)
        path = tmp_path / "host.case"
        F.write_case(path, c["table"], c["rows"][0])
        want, _bits = F.host_step(exe, path)
        got = _host(rays)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        scale = np.maximum(1.0, np.nanmax(np.abs(want), axis=1, keepdims=True))
        err = np.nan_to_num(np.abs(got - want) / scale)
        print(f"{name}: device vs host {err.max():.3g}")
        assert err.max() <= 1e-13, (name, err.max(axis=1))


def test_range_walking_entries_refuse_and_launch_nothing(engines):
    """OL_EUNSUPPORTED (-2) from every existing entry point whose range holds the Forbes row -- a
    return code, not a fault -- with every buffer it was handed left as it was."""
    eng = engines("q2d_norm12_default")
    lib, h = eng.lib, eng._handle
    n = 64
    buf = torch.full((40, n), 3.0, dtype=torch.float64, device=DEV)
    ints = torch.full((64,), 5, dtype=torch.int32, device=DEV)
    rays = (C.c_void_p * 8)(*[buf[k].data_ptr() for k in range(8)])
    three = (C.c_void_p * 3)(*[buf[8 + k].data_ptr() for k in range(3)])
    six = (C.c_void_p * 6)(*[buf[12 + k].data_ptr() for k in range(6)])
    rec, status, stream = buf[20:].data_ptr(), ints[:1].data_ptr(), eng._stream()
    rg, wp = _capi.RaygenParams(), _capi.WavefrontParams()
    inp = _capi.RaygenInputs()
    inp.px = inp.py = buf[18].data_ptr()
    cell = _capi.SpotCell()
    aim = _capi.AimParams(1.0, 1.0, 1e-6, 1, 1)
    last = eng.num_surfaces - 1
    with torch.cuda.device(eng.device):
        calls = {
            "ol_trace": lib.ol_trace(h, 1, n, rays, 0, rec, n, None, 0, last, 1, status, stream),
            "ol_trace one": lib.ol_trace(h, 0, n, rays, 0, None, 0, None, 1, 1, 1, status, stream),
            "ol_trace_ex": lib.ol_trace_ex(h, 1, n, rays, 0, rec, n, None, 0, last, 1, status,
                                           None, stream),
            "ol_newton_count": lib.ol_newton_count(h, 1, n, rays, 0, 0, last, ints.data_ptr(), 0,
                                                   stream),
            "ol_trace_generate": lib.ol_trace_generate(h, 1, n, C.byref(rg), C.byref(inp), 0, rec,
                                                       n, None, None, 0, status, None, stream),
            "ol_trace_spot": lib.ol_trace_spot(h, 1, n, C.byref(rg), C.byref(inp), 0.0, 0.0, 0,
                                               three, buf[19].data_ptr(), status, stream),
            "ol_trace_spot_batch": lib.ol_trace_spot_batch(h, 1, n, C.byref(rg), C.byref(inp), 1,
                                                           C.byref(cell), None, 0,
                                                           buf[19].data_ptr(), status, stream),
            "ol_trace_opd": lib.ol_trace_opd(h, 1, n, C.byref(rg), C.byref(inp), C.byref(wp), 0,
                                             buf[8].data_ptr(), buf[9].data_ptr(), three,
                                             buf[19].data_ptr(), status, stream),
            "ol_wavefront_reference": lib.ol_wavefront_reference(
                h, 1, C.byref(rg), C.byref(inp), C.byref(wp), 0.0, 0, 0, buf[19].data_ptr(),
                buf[11].data_ptr(), status, stream),
            "ol_trace_opd_dev": lib.ol_trace_opd_dev(h, 1, n, C.byref(rg), C.byref(inp),
                                                     buf[19].data_ptr(), 0, buf[8].data_ptr(),
                                                     buf[9].data_ptr(), three, buf[19].data_ptr(),
                                                     status, stream),
            "ol_aim_rays": lib.ol_aim_rays(h, n, 0, 0, last, C.byref(aim), C.byref(inp), None, six,
                                           None, status, stream),
        }
        # in front of the row the range is an ordinary one
        ok = lib.ol_trace(h, 1, n, rays, 0, None, 0, None, 0, 0, 1, status, stream)
    torch.cuda.synchronize()
    assert ok == 0
    assert all(rc == -2 for rc in calls.values()), calls
    assert bool((buf == 3.0).all()) and bool((ints == 5).all())
    with pytest.raises(_capi.HipExtensionError, match="Forbes surface"):
        _capi.check(lib.ol_trace(h, 1, n, rays, 0, rec, n, None, 0, last, 1, status, stream),
                    "ol_trace", lib)
    # the Python layers: a polarised launch and the spot epilogue over such a range are refused
    with pytest.raises(ValueError, match="Forbes"):
        eng.trace([buf[k] for k in range(8)], 0, record=False, first=0, last=last,
                  prt=torch.zeros((9, n), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="not a Forbes row"):
        eng.trace_forbes([buf[k] for k in range(8)], 2, 0, write_rays=True)
    with torch.cuda.device(eng.device):
        rc = lib.ol_trace_forbes(h, 1, n, rays, 0, None, 0, 2, 1, status, stream)
    assert rc == -1 and b"not a Forbes surface" in lib.ol_last_error()


def test_status_bits_and_nan_pattern(engines):
    c = F.case("q_norm12_tight")
    eng = engines("q_norm12_tight")
    rows = np.repeat(c["rows"][0][:, :1], 3, axis=1)
    rows[1, 1] = 500.0                    # misses the base conic: NaN, and only that ray
    rays = _dev(rows)
    assert eng.trace_forbes(rays, F.FORBES, 0, write_rays=True) == 0
    got = _host(rays)
    assert np.isnan(got[:6, 1]).all() and not np.isnan(got[:, [0, 2]]).any()
    np.testing.assert_array_equal(got[:, 0], got[:, 2])
    np.testing.assert_array_equal(np.isnan(got[:, 0]), np.isnan(c["rows"][F.FORBES][:, 0]))
    # glass to air at a steep angle: total internal reflection keeps the position, loses the
    # direction and raises the informational bit -- unless the trace goes on behind the surface
    from optiland_amd.engine import HipSystem
    tir = S.SystemTable.from_json(c["table"].to_json())
    tir.optics["n1"][F.FORBES], tir.optics["n2"][F.FORBES] = 1.8, 1.0
    steep = c["rows"][0][:, :1].copy()
    steep[3:6, 0] = [0.0, np.sin(1.0), np.cos(1.0)]
    steep[1, 0] = steep[2, 0] * np.tan(1.0)
    eng2 = HipSystem(tir, DEV)
    try:
        for midrange, want in ((False, S.STATUS_NAN_DIRECTION), (True, 0)):
            rays = _dev(steep)
            assert eng2.trace_forbes(rays, F.FORBES, 0, write_rays=True, midrange=midrange) == want
            got = _host(rays)
            assert np.isnan(got[3:6, 0]).all() and not np.isnan(got[:3, 0]).any()
    finally:
        eng2.close()
