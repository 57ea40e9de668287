"""Grid-sag surfaces on the MI355X (`ol_trace_grid_sag`, csrc/grid_sag.hip) against the
reference's recorded traces (tests/golden/grid_sag.npz, tools/make_golden_grid_sag.py): the
one-surface launch in fp64 and fp32 against every case at both tolerances and against the host run
of its own source, the split of `HipSystem.trace` (fused run, grid-sag surface, fused run), record
row, write-back and mid-range flag, the status bit, bundle sizes that are no multiple of the
workgroup between guard planes, the C entry called directly and the live drop-in.  Fixture tables
only; bounds: tests/_grid_sag.py.

Every index the kernel forms into the ray planes is i < n on planes of n elements (a record row
of stride >= n); the coordinate and node loads are clamped into the block before the load
(csrc/grid_sag_device.h; the sanitized host run of tests/test_grid_sag_cpu.py holds that); no test
hands the launch anything else.  ~470 rays per case.

Measured on the MI355X (profiles/grid_sag.txt): every case within 0.0013 of the 1e-12 bound in fp64
at tol = 1e-12 and within 0.004 of the contract in fp32; device against the host run 8.9e-16 (4
ulp; the bound below is 16); the live optic under enable() within 0.0008 of the 1e-12 bound of the
reference's own trace in the same process; 55 tests in seconds."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

from optiland_amd import _capi
from optiland_amd import system as S
from tests import _grid_sag as G
from tests import _live

pytestmark = pytest.mark.gpu
REF = _live.reference_root() or _live.STAGED
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "optiland")),
                                     reason="reference package not present")

DEV = "cuda"
ROW = G.GRID
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
# Device against the host run of the same source, fp64, as a share of the plane's scale.  The two
# differ in the hardware's division, square root and reciprocal square root only, each within an
# ulp of the IEEE result the host takes.  One Newton update holds two such quotients in sequence
# (tx, ty of the cell, then dt = f / f'), the hit x + t L rounds once more, the normal takes an
# rsqrt and Snell's law a sqrt behind it: six roundings that may differ, each carried into the next
# with a factor of order 1 (the cell's slope is < 0.3, the index ratio < 1.6).  16 ulp = 3.6e-15
# is that chain with a factor 2-3 to spare; forbes got 9e-16 and phase 2.2e-16 the same way.
DEVICE_VS_HOST = 16 * 2.220446049250313e-16


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from optiland_amd.engine import HipSystem
    made = {}

    def get(name, tol="tight"):
        if (name, tol) not in made:
            made[name, tol] = HipSystem(G.case(name, tol)["table"], DEV)
        return made[name, tol]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def hostgrid():
    b = G._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return b.build()


def _dev(planes, dtype=np.float64):
    return [torch.as_tensor(np.array(p), dtype=TORCH[dtype], device=DEV) for p in planes]


def _host(planes):
    return np.stack([p.double().cpu().numpy() for p in planes])


def _check(got, c, dtype, key, what):
    """`got` (8, n) against the case's `key` row with the bounds of the issue: fp64 within 1e-12
    at tol = 1e-12, the contract otherwise; NaN masks equal."""
    tight = dtype is np.float64 and c["tol"] == G.TOLS["tight"]
    scale = G.scale_of(np.stack([c["before"], c["after"], c["lens"]]))
    G.compare(got, c[key], dtype, scale, f"{what} tol {c['tol']:g}", report=print)
    if tight:
        G.compare(got, c[key], dtype, scale, f"{what} tol {c['tol']:g}", tight=True, report=print)


@pytest.mark.parametrize("tol", list(G.TOLS))
@pytest.mark.parametrize("name", list(G.CASES))
def test_trace_grid_sag_against_every_case(name, tol, engines):
    """The recorded row and the written-back state of one launch, fp64 and fp32, against the
    fixture; the status bit exactly when the case has NaN rays."""
    c = G.case(name, tol)
    eng = engines(name, tol)
    assert eng.can_trace_grid_sag() and eng.table.grid_sag_rows == (ROW,)
    n = c["after"].shape[1]
    for dtype in (np.float64, np.float32):
        rays = _dev(c["before"], dtype)
        row = torch.full((8, n + 5), -7.0, dtype=TORCH[dtype], device=DEV)
        status = eng.trace_grid_sag(rays, ROW, 0, record_row=row, write_rays=True)
        assert bool(status & S.STATUS_NAN_DIRECTION) == (name in G.NAN_CASES)
        assert status & ~S.STATUS_NAN_DIRECTION == 0
        got = _host(rays)
        np.testing.assert_array_equal(got, row[:, :n].double().cpu().numpy())
        assert bool((row[:, n:] == -7.0).all())          # nothing behind the n rays is written
        _check(got, c, dtype, "after", name)


@pytest.mark.parametrize("tol", list(G.TOLS))
@pytest.mark.parametrize("name", list(G.CASES))
def test_the_split_of_trace_equals_the_fixture(name, tol, engines):
    """`HipSystem.trace` over [stop, image] from the state in front of the grid-sag surface: a
    fused run (the stop plane, where the rays already are), the grid-sag launch, a fused run; the
    record block is one tensor; its grid-sag row and its last row against the fixture."""
    c = G.case(name, tol)
    eng = engines(name, tol)
    n, last = c["after"].shape[1], eng.num_surfaces - 1
    for dtype in (np.float64, np.float32):
        start = _dev(c["before"], dtype)
        res = eng.trace(start, 0, record=True, first=ROW - 1, last=last, check_status=False)
        assert isinstance(res.record, torch.Tensor) and res.record.shape[:2] == (last - ROW + 2, 8)
        got = res.record[:, :, :n].double().cpu().numpy()
        np.testing.assert_array_equal(_host(start), c["before"].astype(dtype))   # not written
        np.testing.assert_array_equal(got[0], c["before"].astype(dtype))          # the stop: t = 0
        _check(got[1], c, dtype, "after", name + " split")
        _check(got[-1], c, dtype, "lens", name + " lens")
        final = [t.clone() for t in start]
        eng.trace(final, 0, record=False, first=ROW, last=last, check_status=False)
        assert torch.equal(torch.stack(final).view(torch.uint8),
                           res.record[-1, :, :n].contiguous().view(torch.uint8))


def test_device_equals_the_host_run_of_its_source(engines, hostgrid, tmp_path):
    """fp64, every case at both tolerances: the device against the host build of the same header
    (the one test of this file that needs a host compiler)."""
    worst = 0.0
    for name in G.CASES:
        for tol in G.TOLS:
            c = G.case(name, tol)
            rays = _dev(c["before"])
            engines(name, tol).trace_grid_sag(rays, ROW, 0, write_rays=True)
            got = _host(rays)
            path = tmp_path / "host.case"
            G.write_case(path, c["table"], c["before"])
            host, _bits = G.host_step(hostgrid, path)
            assert np.array_equal(np.isnan(got), np.isnan(host))
            span = np.maximum(1.0, np.nanmax(np.abs(host), axis=1, keepdims=True))
            err = np.nan_to_num(np.abs(got - host) / span)
            print(f"{name} tol {c['tol']:g}: device vs host {err.max():.3g}")
            worst = max(worst, float(err.max()))
            assert err.max() <= DEVICE_VS_HOST, (name, tol, err.max(axis=1))
    print(f"device vs host, worst of all cases: {worst:.3g}")


def test_record_row_write_back_and_midrange(engines):
    """A record row inside a block whose stride is larger than n; write_rays with and without a
    record row; without write_rays the eight planes stay as they were -- as for
    `trace_forbes`."""
    name = "tilted"
    c = G.case(name)
    eng = engines(name)
    n = c["after"].shape[1]
    block = torch.full((3, 8, n + 33), -7.0, dtype=torch.float64, device=DEV)
    rays = _dev(c["before"])
    assert eng.trace_grid_sag(rays, ROW, 0, record_row=block[1], write_rays=False) == 0
    np.testing.assert_array_equal(_host(rays), c["before"])               # not written
    got = block[1, :, :n].cpu().numpy()
    _check(got, c, np.float64, "after", "record row")
    assert bool((block[0] == -7.0).all()) and bool((block[2] == -7.0).all()) \
        and bool((block[1, :, n:] == -7.0).all())
    eng.trace_grid_sag(rays, ROW, 0, write_rays=True)                     # in place, no record row
    np.testing.assert_array_equal(_host(rays), got)
    rays = _dev(c["before"])
    block.fill_(-7.0)
    eng.trace_grid_sag(rays, ROW, 0, record_row=block[2], write_rays=True, midrange=True)
    np.testing.assert_array_equal(_host(rays), got)
    np.testing.assert_array_equal(block[2, :, :n].cpu().numpy(), got)
    with pytest.raises(ValueError, match="nothing to write"):
        eng.trace_grid_sag(rays, ROW, 0, write_rays=False)
    with pytest.raises(ValueError, match="not a grid-sag row"):
        eng.trace_grid_sag(rays, ROW - 1, 0, write_rays=True)


def test_status_bit_when_and_only_when_rays_left_the_grid(engines):
    """STATUS_NAN_DIRECTION: set by a bundle with NaN rays, not with OL_TRACE_MIDRANGE, not by the
    part of the same bundle that stays on the grid, not by a bundle of another case."""
    c = G.case("narrow")
    eng = engines("narrow")
    lost = np.isnan(c["after"][0])
    assert 0 < lost.sum() < lost.size
    for dtype in (np.float64, np.float32):
        assert eng.trace_grid_sag(_dev(c["before"], dtype), ROW, 0, write_rays=True) \
            == S.STATUS_NAN_DIRECTION
        assert eng.trace_grid_sag(_dev(c["before"], dtype), ROW, 0, write_rays=True,
                                  midrange=True) == 0
        assert eng.trace_grid_sag(_dev(c["before"][:, ~lost], dtype), ROW, 0,
                                  write_rays=True) == 0
        rays = _dev(c["before"][:, lost], dtype)
        assert eng.trace_grid_sag(rays, ROW, 0, write_rays=True) == S.STATUS_NAN_DIRECTION
        assert np.isnan(_host(rays)[:6]).all()
        # the whole trace: the grid-sag launch is mid-range there and raises nothing else
        res = eng.trace(_dev(c["before"], dtype), 0, record=False, first=ROW,
                        last=eng.num_surfaces - 1)
        assert res.status & ~S.STATUS_NAN_DIRECTION == 0
    c = G.case("uniform")
    assert engines("uniform").trace_grid_sag(_dev(c["before"]), ROW, 0, write_rays=True) == 0


@pytest.mark.parametrize("n", [1, 63, 257])
def test_odd_bundle_sizes_write_no_lane_beyond_n(n, engines):
    """1, 63 and 257 rays (less than a wave, a wave short of one lane, four workgroups and one
    lane): the ray planes and the record row lie between guard planes and carry guard elements
    behind n; nothing but the n rays is written, and those are right."""
    c = G.case("narrow")            # (with rays that leave the grid among them)
    eng = engines("narrow")
    idx = np.linspace(0, c["before"].shape[1] - 1, n).astype(int)   # inner and outer rings
    before, want = c["before"][:, idx], c["after"][:, idx]
    for dtype in (np.float64, np.float32):
        pad = 64
        buf = torch.full((10, n + pad), -7.0, dtype=TORCH[dtype], device=DEV)
        rec = torch.full((10, n + pad), -9.0, dtype=TORCH[dtype], device=DEV)
        buf[1:9, :n] = torch.as_tensor(before, dtype=TORCH[dtype], device=DEV)
        planes = [buf[1 + k, :n] for k in range(8)]
        assert all(p.is_contiguous() for p in planes)
        eng.trace_grid_sag(planes, ROW, 0, record_row=rec[1:9], write_rays=True,
                           check_status=False)
        torch.cuda.synchronize()
        got = buf[1:9, :n].double().cpu().numpy()
        case = dict(c, before=before, after=want, lens=want)
        _check(got, case, dtype, "after", f"n={n}")
        np.testing.assert_array_equal(got, rec[1:9, :n].double().cpu().numpy())
        assert bool((buf[0] == -7.0).all()) and bool((buf[9] == -7.0).all())
        assert bool((buf[:, n:] == -7.0).all())
        assert bool((rec[0] == -9.0).all()) and bool((rec[9] == -9.0).all())
        assert bool((rec[:, n:] == -9.0).all())


@pytest.mark.parametrize("name", ["uniform", "narrow"])
def test_the_256_thread_launch_checks_every_lane(name, engines):
    """65 537 rays, tiled from the case's bundle: the launcher's switch from 64-thread to
    256-thread workgroups (65 536 rays and more) and one lane of a last workgroup, every lane
    against the fixture; with the narrow case, NaN rays in every wave and the status bit from one
    lane per wave."""
    c = G.case(name)
    eng = engines(name)
    n = 65537
    idx = np.arange(n) % c["before"].shape[1]
    case = dict(c, before=c["before"][:, idx], after=c["after"][:, idx], lens=c["lens"][:, idx])
    for dtype in (np.float64, np.float32):
        rays = _dev(case["before"], dtype)
        row = torch.full((8, n + 3), -7.0, dtype=TORCH[dtype], device=DEV)
        status = eng.trace_grid_sag(rays, ROW, 0, record_row=row, write_rays=True)
        assert status == (S.STATUS_NAN_DIRECTION if name in G.NAN_CASES else 0)
        got = _host(rays)
        np.testing.assert_array_equal(got, row[:, :n].double().cpu().numpy())
        assert bool((row[:, n:] == -7.0).all())
        _check(got, case, dtype, "after", f"{name} n={n}")


def test_c_entry_directly(engines):
    """OL_OK, the status word stays 0 on a clean bundle, a wrong-kind surface gets its refusal
    text, a range entry refuses the grid-sag row and launches nothing, a polarised trace is
    refused in Python."""
    c = G.case("coated")
    eng = engines("coated")
    lib, h = eng.lib, eng._handle
    n = c["after"].shape[1]
    rays_t = _dev(c["before"])
    rays = (C.c_void_p * 8)(*[t.data_ptr() for t in rays_t])
    row = torch.full((8, n), -7.0, dtype=torch.float64, device=DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = eng._stream()
    with torch.cuda.device(eng.device):
        rc = lib.ol_trace_grid_sag(h, _capi.F64, n, rays, 0, row.data_ptr(), n, ROW, 0,
                                   word.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.ol_last_error()
        assert int(word.item()) == 0
        _check(row.cpu().numpy(), c, np.float64, "after", "C entry")
        np.testing.assert_array_equal(_host(rays_t), c["before"])     # no OL_TRACE_WRITE_RAYS
        rc = lib.ol_trace_grid_sag(h, _capi.F64, n, rays, 0, row.data_ptr(), n, ROW + 1, 0,
                                   word.data_ptr(), stream)
        assert rc == -1 and lib.ol_last_error() == (
            b"ol_trace_grid_sag: surface 3 is not a grid-sag surface (geometry kind 1): trace it "
            b"with ol_trace")
        keep = row.clone()
        last = eng.num_surfaces - 1
        rc = lib.ol_trace(h, _capi.F64, n, rays, 0, None, 0, None, 0, last, 1, word.data_ptr(),
                          stream)
        assert rc == -2 and b"surface 2 is a grid-sag surface" in lib.ol_last_error()
        torch.cuda.synchronize()
    assert torch.equal(row.view(torch.uint8), keep.view(torch.uint8))
    np.testing.assert_array_equal(_host(rays_t), c["before"])
    with pytest.raises(ValueError, match="grid-sag surfaces"):
        eng.trace(rays_t, 0, record=False, prt=torch.zeros((9, n), dtype=torch.float64, device=DEV))


@needs_reference
@pytest.mark.parametrize("edit", [dict(), dict(half=4.6)], ids=["wide", "narrow"])
def test_live_optic_under_enable_is_one_launch_and_equals_the_reference(edit, monkeypatch):
    """The reference's `Optic.trace` of a grid-sag singlet on the torch backend on the device:
    under `enable()` the surface is ONE `ol_trace_grid_sag` launch and no surface goes to the
    reference's own trace; under `enable(grid_sags=False)` it is the reference's surface again;
    the two traces of the same process agree -- at tol = 1e-12 to the fp64 bound, the rays that
    leave the narrow grid NaN in both."""
    from optiland_amd import integration as I
    from optiland_amd.engine import HipSystem

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    be = _live.import_reference()
    launches = []
    inner = HipSystem.trace_grid_sag

    def counted(self, rays, surface, *a, **k):
        launches.append(int(surface))
        return inner(self, rays, surface, *a, **k)

    monkeypatch.setattr(HipSystem, "trace_grid_sag", counted)
    was = I._SG["grid_sags"]
    be.set_backend("torch")
    be.set_device("cuda")
    be.set_precision("float64")

    def recorded(lens):
        return np.stack([np.stack([np.asarray(be.to_numpy(getattr(s, k)), dtype=np.float64)
                                   .reshape(-1) for k in ("x", "y", "z", "L", "M", "N",
                                                          "intensity", "opd")])
                         for s in lens.surfaces.surfaces])

    try:
        lens = G.lens(G.TOLS["tight"], **edit)
        I.enable(grid_sags=True)
        foreign, served = I._SG["foreign"], I._SG["count"]
        lens.trace(0.0, 1.0, G.WAVELENGTH, 12, "hexapolar")
        got = recorded(lens)
        assert launches == [ROW]
        assert I._SG["foreign"] == foreign and I._SG["count"] == served + 1
        I.enable(grid_sags=False)
        lens.trace(0.0, 1.0, G.WAVELENGTH, 12, "hexapolar")
        want = recorded(lens)
        assert launches == [ROW] and I._SG["foreign"] == foreign + 1
        assert got.shape == want.shape and got.shape[2] == 469
        assert bool(np.isnan(want[ROW, 0]).any()) == bool(edit)
        # (the reference's hexapolar rings are not turned off the grid lines as the fixture's
        # are: a hit within rounding of a line -- 5 cos(60 deg) beside the node 2.5 -- may take the
        # neighbour cell's slope.  Both traces are fp64: the hit is good to a few ulp of a
        # coordinate of up to 8 mm, 1.8e-15 each; 64 of them is the margin, 1.1e-13 mm)
        table = G.packed(lens)
        d = G.grid_line_distance(table, ROW, want[ROW])
        away = ~((d > 0) & (d < 64 * 8.0 * 2.220446049250313e-16)).any(axis=0)
        # (the six-fold rings put up to 28 rays there: two per ring at x = r cos(90 deg) ~ 1e-16
        # beside the node 0, four of the last ring at 2.5)
        assert away.sum() >= away.size - 32
        G.compare(got[:, :, away], want[:, :, away], np.float64, G.scale_of(want),
                  "live grid-sag singlet", tight=True, report=print)
    finally:
        I.enable(grid_sags=True)
        I.disable()
        I._SG["grid_sags"] = was
        be.set_backend("numpy")
