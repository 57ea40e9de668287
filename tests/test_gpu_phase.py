"""Phase-profile surfaces on the MI355X (`ol_trace_phase`, csrc/phase.hip) against the
reference's recorded traces (tests/golden/phase.npz, tools/make_golden_phase.py): the one-surface
launch in fp64 and fp32 against every case and against the host run of its own source, the launch
sizes around the wave, the workgroup and the launcher's switch of block size, record row and
write-back, an evanescent ray's zero intensity without a status bit, the whole optic through
`HipSystem.trace` (fused run, phase plane, fused run) and the C entry called directly.  Fixture
tables only; bounds: tests/_phase.py.

Every index the kernel forms into the ray planes is i < n on planes of n elements (a record row
of stride >= n); the four gathers of a gridded profile are clamped into the node block before the
load (csrc/phase_device.h); no test hands the launch anything else.

Measured on the MI355X (profiles/phase.txt): every case within 0.00103 of the 1e-12 bound in fp64
and 0.0023 of the contract in fp32; the whole optic within 0.0028 of the contract in fp32 (the
tilted case); device against the host run 2.2e-16; the live optic under enable() within 0.0008 of the 1e-12
bound of the reference's own trace in the same process; 49 tests in about 12 s (the two live
optics about 4 s each: importing the reference and its first traces)."""

import ctypes as C

import numpy as np
import pytest
import torch

import os

from optiland_amd import _capi
from optiland_amd import system as S
from tests import _live
from tests import _phase as P

pytestmark = pytest.mark.gpu
REF = _live.reference_root() or _live.STAGED
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "optiland")),
                                     reason="reference package not present")

DEV = "cuda"
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
# device against the host run of the same source, fp64, as a share of the plane's scale: the two
# differ in the hardware's division and square root only -- the project's figure for that
# comparison (tests/test_gpu_forbes.py, tests/test_gpu_grating.py)
DEVICE_VS_HOST = 1e-13


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from optiland_amd.engine import HipSystem
    made = {}

    def get(name):
        if name not in made:
            made[name] = HipSystem(P.case(name)["table"], DEV)
        return made[name]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def hostphase():
    b = P._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return b.build()


def _dev(planes, dtype=np.float64):
    return [torch.as_tensor(np.array(p), dtype=TORCH[dtype], device=DEV)
            for p in planes]


def _host(planes):
    return np.stack([p.double().cpu().numpy() for p in planes])


def _scale(c):
    return P.scale_of(c["rows"][:c["g"] + 1])


@pytest.mark.parametrize("name", list(P.CASES))
def test_trace_phase_against_every_case(name, engines):
    """The recorded row and the written-back state of one launch, fp64 and fp32, against the
    fixture -- fp64 also at 1e-12.  Needs nothing but the device and the fixture."""
    c = P.case(name)
    g, wl = c["g"], c["wl"]
    eng = engines(name)
    assert eng.can_trace_phase() and eng.table.phases == (g,)
    before, want = c["rows"][g - 1], c["rows"][g]
    n = want.shape[1]
    for dtype in (np.float64, np.float32):
        rays = _dev(before, dtype)
        row = torch.full((8, n + 5), -7.0, dtype=TORCH[dtype], device=DEV)
        status = eng.trace_phase(rays, g, wl, record_row=row, write_rays=True)
        assert status == 0
        got = _host(rays)
        np.testing.assert_array_equal(got, row[:, :n].double().cpu().numpy())
        assert bool((row[:, n:] == -7.0).all())          # nothing behind the n rays is written
        P.compare(got, want, dtype, _scale(c), name, report=print)
        if dtype is np.float64:
            P.compare(got, want, dtype, _scale(c), name, tight=True, report=print)


def test_device_equals_the_host_run_of_its_source(engines, hostphase, tmp_path):
    """fp64, every case: the device against the host build of the same header (the one test of
    this file that needs a host compiler)."""
    for name in P.CASES:
        c = P.case(name)
        g, wl = c["g"], c["wl"]
        before = c["rows"][g - 1]
        rays = _dev(before)
        engines(name).trace_phase(rays, g, wl, write_rays=True)
        got = _host(rays)
        path = tmp_path / "host.case"
        P.write_case(path, c["table"], before, g, wl_index=wl)
        host, _bits = P.host_step(hostphase, path)
        assert np.array_equal(np.isnan(got), np.isnan(host))
        span = np.maximum(1.0, np.nanmax(np.abs(host), axis=1, keepdims=True))
        err = np.nan_to_num(np.abs(got - host) / span)
        print(f"{name}: device vs host {err.max():.3g}")
        assert err.max() <= DEVICE_VS_HOST, (name, err.max(axis=1))


@pytest.fixture(scope="module")
def big_reference(engines):
    """65 537 rays tiled from the 1027-ray sets, and their expected rows: computed once."""
    out = {}
    for name in P.BIG_CASES:
        c = P.case(name)
        m = c["big_in"].shape[1]
        idx = np.arange(65537) % m
        out[name] = (c["big_in"][:, idx], c["big_out"][:, idx])
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 65537])
@pytest.mark.parametrize("name", list(P.BIG_CASES))
def test_launch_sizes_check_every_lane(name, n, engines, big_reference):
    """The wave edge (63 / 64 / 65), several workgroups (257) and the launcher's switch from
    64-thread to 256-thread workgroups (65 536 rays and more): every lane, on the radial row and
    on the grid row with its hits outside the grid."""
    c = P.case(name)
    g, wl = c["g"], c["wl"]
    eng = engines(name)
    before, want = (a[:, :n] for a in big_reference[name])
    for dtype in (np.float64, np.float32):
        rays = _dev(before, dtype)
        assert eng.trace_phase(rays, g, wl, write_rays=True) == 0
        got = _host(rays)
        P.compare(got, want, dtype, _scale(c), f"{name} n={n}",
                  report=print if n == 65537 else None)
        if dtype is np.float64:
            P.compare(got, want, dtype, _scale(c), f"{name} n={n}", tight=True)


def test_record_row_and_write_back(engines):
    """A record row inside a block whose stride is larger than n; write_rays with and without a
    record row; without write_rays the eight planes stay as they were."""
    name = "tilted"
    c = P.case(name)
    g = c["g"]
    eng = engines(name)
    before, want = c["rows"][g - 1], c["rows"][g]
    n = want.shape[1]
    block = torch.full((3, 8, n + 33), -7.0, dtype=torch.float64, device=DEV)
    rays = _dev(before)
    eng.trace_phase(rays, g, 0, record_row=block[1], write_rays=False)
    np.testing.assert_array_equal(_host(rays), before)               # not written
    got = block[1, :, :n].cpu().numpy()
    P.compare(got, want, np.float64, _scale(c), "record row", tight=True)
    assert bool((block[0] == -7.0).all()) and bool((block[2] == -7.0).all()) \
        and bool((block[1, :, n:] == -7.0).all())
    eng.trace_phase(rays, g, 0, write_rays=True)                     # in place, no record row
    np.testing.assert_array_equal(_host(rays), got)
    rays = _dev(before)
    block.fill_(-7.0)
    eng.trace_phase(rays, g, 0, record_row=block[2], write_rays=True)
    np.testing.assert_array_equal(_host(rays), got)
    np.testing.assert_array_equal(block[2, :, :n].cpu().numpy(), got)
    with pytest.raises(ValueError, match="nothing to write"):
        eng.trace_phase(rays, g, 0, write_rays=False)
    with pytest.raises(ValueError, match="not a phase row"):
        eng.trace_phase(rays, g - 1, 0, write_rays=True)


@pytest.mark.parametrize("name", list(P.TIR_CASES))
def test_an_evanescent_ray_is_clipped_and_keeps_a_direction(name):
    """Intensity 0, a finite unit direction along the surface and NO status bit -- also when the
    phase plane is the LAST surface of the table, and with and without midrange."""
    from optiland_amd.engine import HipSystem

    c = P.case(name)
    g = c["g"]
    full = c["table"]
    cut = S.SystemTable(surfaces=full.surfaces[:g + 1].copy(), coeffs=full.coeffs.copy(),
                        optics=full.optics[:g + 1].copy(), wavelengths=full.wavelengths.copy())
    eng = HipSystem(cut, DEV)
    try:
        assert eng.table.phases == (g,) and eng.num_surfaces == g + 1
        want = c["rows"][g]
        tir = P.radicand(full, g, c["rows"][g - 1], want) < 0
        assert 0.1 <= tir.mean() <= 0.9
        for dtype in (np.float64, np.float32):
            for midrange in (False, True):
                rays = _dev(c["rows"][g - 1], dtype)
                assert eng.trace_phase(rays, g, 0, write_rays=True, midrange=midrange) == 0
                got = _host(rays)
                assert np.isfinite(got).all()
                assert np.array_equal(got[6] == 0.0, tir)
                assert np.all(got[5][tir] == 0.0)
                norm = np.sqrt((got[3:6] ** 2).sum(axis=0))
                assert np.abs(norm - 1.0).max() <= (1e-12 if dtype is np.float64 else 1e-5)
        res = eng.trace(_dev(c["rows"][0]), 0, record=True)
        assert res.status == 0
        P.compare(res.record[:, :, :res.n].cpu().numpy(), c["rows"][:g + 1], np.float64,
                  _scale(c), name + " cut", tight=True)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(P.CASES))
def test_whole_optic_equals_the_fixture(name, engines):
    """`HipSystem.trace` over the whole table (fused run, phase plane, fused run) against the
    reference's records; the record block is one tensor.  In the TIR cases the rows up to the
    phase plane: behind it an evanescent ray has N = 0 exactly and the image plane's -z / N is
    inf / NaN in the reference as well."""
    c = P.case(name)
    g, wl = c["g"], c["wl"]
    eng = engines(name)
    n, last = c["rows"].shape[2], c["rows"].shape[0] - 1
    upto = g + 1 if name in P.TIR_CASES else last + 1
    scale = P.scale_of(c["rows"][:upto])
    for dtype in (np.float64, np.float32):
        start = _dev(c["rows"][0], dtype)
        res = eng.trace(start, wl, record=True, first=0, last=last, check_status=False)
        assert isinstance(res.record, torch.Tensor) and res.record.shape[:2] == (last + 1, 8)
        got = res.record[:, :, :n].double().cpu().numpy()
        np.testing.assert_array_equal(_host(start), c["rows"][0].astype(dtype))   # not written
        P.compare(got[:upto], c["rows"][:upto], dtype, scale, name, report=print)
        if dtype is np.float64:
            P.compare(got[:upto], c["rows"][:upto], dtype, scale, name, tight=True, report=print)
        final = [t.clone() for t in start]
        eng.trace(final, wl, record=False, first=0, last=last, check_status=False)
        assert torch.equal(torch.stack(final).view(torch.uint8),
                           res.record[last, :, :n].contiguous().view(torch.uint8))


def test_c_entry_directly(engines):
    """OL_OK, the status word stays 0, a wrong-kind surface gets its refusal text, a range entry
    refuses the phase row and launches nothing; the height case takes its scale from the
    wavelength index."""
    c = P.case("height_blue")
    g, wl = c["g"], c["wl"]
    assert wl == 1
    eng = engines("height_blue")
    lib, h = eng.lib, eng._handle
    before, want = c["rows"][g - 1], c["rows"][g]
    n = want.shape[1]
    rays_t = _dev(before)
    rays = (C.c_void_p * 8)(*[t.data_ptr() for t in rays_t])
    row = torch.full((8, n), -7.0, dtype=torch.float64, device=DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = eng._stream()
    um = P.WAVELENGTHS[wl]
    with torch.cuda.device(eng.device):
        rc = lib.ol_trace_phase(h, _capi.F64, n, rays, wl, um, row.data_ptr(), n, g, 0,
                                word.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.ol_last_error()
        assert int(word.item()) == 0
        P.compare(row.cpu().numpy(), want, np.float64, _scale(c), "C entry", tight=True)
        np.testing.assert_array_equal(_host(rays_t), before)          # no OL_TRACE_WRITE_RAYS
        # the other wavelength index is another scale: another answer
        rc = lib.ol_trace_phase(h, _capi.F64, n, rays, 0, um, row.data_ptr(), n, g, 0,
                                word.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0 and np.abs(row.cpu().numpy()[3:6] - want[3:6]).max() > 1e-4
        rc = lib.ol_trace_phase(h, _capi.F64, n, rays, wl, um, row.data_ptr(), n, g - 1, 0,
                                word.data_ptr(), stream)
        assert rc == -1 and lib.ol_last_error() == (
            b"ol_trace_phase: surface 1 is not a phase surface (geometry kind 0): trace it with "
            b"ol_trace")
        rc = lib.ol_trace_phase(h, _capi.F64, n, rays, wl, 0.0, row.data_ptr(), n, g, 0,
                                word.data_ptr(), stream)
        assert rc == -1 and b"wavelength_um 0 must be finite and greater than 0" \
            in lib.ol_last_error()
        keep = row.clone()
        last = eng.num_surfaces - 1
        rc = lib.ol_trace(h, _capi.F64, n, rays, 0, None, 0, None, 0, last, 1, word.data_ptr(),
                          stream)
        assert rc == -2 and b"surface 2 is a phase surface" in lib.ol_last_error()
        torch.cuda.synchronize()
    assert torch.equal(row.view(torch.uint8), keep.view(torch.uint8))
    np.testing.assert_array_equal(_host(rays_t), before)
    with pytest.raises(ValueError, match="phase surfaces"):
        eng.trace(rays_t, 0, record=False, prt=torch.zeros((9, n), dtype=torch.float64, device=DEV))


@needs_reference
@pytest.mark.parametrize("kind", ["radial", "grid"])
def test_live_optic_under_enable_is_one_launch_and_equals_the_reference(kind, monkeypatch):
    """A live reference optic with a phase plane on the torch backend on the device: under
    `enable()` the plane is ONE `ol_trace_phase` launch and no surface goes to the reference's
    own trace; under `enable(phases=False)` it is the reference's surface again; the two traces
    of the same process agree to the fp64 bound."""
    from optiland_amd import integration as I
    from optiland_amd.engine import HipSystem

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    be = _live.import_reference()
    launches = []
    inner = HipSystem.trace_phase

    def counted(self, rays, surface, *a, **k):
        launches.append(int(surface))
        return inner(self, rays, surface, *a, **k)

    monkeypatch.setattr(HipSystem, "trace_phase", counted)
    was = I._SG["phases"]
    be.set_backend("torch")
    be.set_device("cuda")
    be.set_precision("float64")

    def recorded(lens):
        return np.stack([np.stack([np.asarray(be.to_numpy(getattr(s, k)), dtype=np.float64)
                                   .reshape(-1) for k in ("x", "y", "z", "L", "M", "N",
                                                          "intensity", "opd")])
                         for s in lens.surfaces.surfaces])

    try:
        lens = P.lens(kind, material="N-BK7")
        I.enable(phases=True)
        foreign, served = I._SG["foreign"], I._SG["count"]
        lens.trace(0.0, 1.0, P.WAVELENGTH, 6, "hexapolar")
        got = recorded(lens)
        assert launches == [P.PHASE]
        assert I._SG["foreign"] == foreign and I._SG["count"] == served + 1
        I.enable(phases=False)
        lens.trace(0.0, 1.0, P.WAVELENGTH, 6, "hexapolar")
        want = recorded(lens)
        assert launches == [P.PHASE] and I._SG["foreign"] == foreign + 1
        assert got.shape == want.shape and got.shape[2] == 127
        table = P.packed(lens)
        block = P.block_of(table, P.PHASE)
        away = P.grid_line_distance(block, *P.local_hit(table, P.PHASE, want[P.PHASE])) \
            >= P.GRID_MARGIN
        assert away.mean() >= 1 - P.GRID_DROP_CAP
        P.compare(got[:, :, away], want[:, :, away], np.float64, P.scale_of(want), "live " + kind,
                  tight=True, report=print)
    finally:
        I.enable(phases=True)
        I.disable()
        I._SG["phases"] = was
        be.set_backend("numpy")
