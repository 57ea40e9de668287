"""Diffraction gratings on the MI355X (`ol_trace_grating`, csrc/grating.hip) against the
reference's recorded traces (tests/golden/grating.npz, tools/make_golden_grating.py): the
one-surface launch in fp64 and fp32 against every case and against the host run of its own source,
the launch sizes around the wave, the workgroup and the launcher's switch of block size, record
row and write-back, the status bit, the whole optic through `HipSystem.trace` (fused run, grating,
fused run) and the C entry called directly.  Fixture tables only; bounds: tests/_grating.py.

Every index the kernel forms is i < n on planes of n elements (a record row of stride >= n); no
test hands it anything else.

Measured on the MI355X (profiles/grating.txt): every case within 0.0013 of the 1e-12 bound in fp64
(1.3e-9 of the contract) and 0.009 of the contract in fp32; the whole optic within 0.007 / 0.06
(the evanescent cases, whose surviving rays travel far); device against the host run 1.7e-15;
54 tests in about 3 s."""

import ctypes as C

import numpy as np
import pytest
import torch

from optiland_amd import _capi
from optiland_amd import system as S
from tests import _grating as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
# device against the host run of the same source, fp64, as a share of the plane's scale: the two
# differ in the hardware's division and square root only (a few ulp each, some twenty operations
# deep, amplified by at most 1 / (2 sqrt(S / n2^2)) = 5 at the fixture's margin) -- the project's
# figure for that comparison (tests/test_gpu_forbes.py)
DEVICE_VS_HOST = 1e-13


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from optiland_amd.engine import HipSystem
    made = {}

    def get(name):
        if name not in made:
            made[name] = HipSystem(G.case(name)["table"], DEV)
        return made[name]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def hostgrating():
    b = G._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return b.build()


def _dev(planes, dtype=np.float64):
    return [torch.as_tensor(np.array(p), dtype=TORCH[dtype], device=DEV)
            for p in planes]


def _host(planes):
    return np.stack([p.double().cpu().numpy() for p in planes])


def _expect_status(want):
    return S.STATUS_NAN_DIRECTION if np.isnan(want[3]).any() else 0


@pytest.mark.parametrize("name", list(G.CASES))
def test_trace_grating_against_every_case(name, engines):
    """The recorded row and the written-back state of one launch, fp64 and fp32, against the
    fixture -- fp64 also at 1e-12.  Needs nothing but the device and the fixture."""
    c = G.case(name)
    g = c["g"]
    eng = engines(name)
    assert eng.can_trace_grating() and eng.table.gratings == (g,)
    before, want = c["rows"][g - 1], c["rows"][g]
    n = want.shape[1]
    scale = G.scale_of(c["rows"])
    for dtype in (np.float64, np.float32):
        rays = _dev(before, dtype)
        row = torch.full((8, n + 5), -7.0, dtype=TORCH[dtype], device=DEV)
        status = eng.trace_grating(rays, g, 0, record_row=row, write_rays=True)
        assert status == _expect_status(want)
        got = _host(rays)
        np.testing.assert_array_equal(got, row[:, :n].double().cpu().numpy())
        assert bool((row[:, n:] == -7.0).all())          # nothing behind the n rays is written
        G.compare(got, want, dtype, scale, name, report=print)
        if dtype is np.float64:
            G.compare(got, want, dtype, scale, name, tight=True, report=print)


def test_device_equals_the_host_run_of_its_source(engines, hostgrating, tmp_path):
    """fp64, every case: the device against the host build of the same header (the one test of
    this file that needs a host compiler)."""
    for name in G.CASES:
        c = G.case(name)
        g = c["g"]
        before = c["rows"][g - 1]
        rays = _dev(before)
        engines(name).trace_grating(rays, g, 0, write_rays=True)
        got = _host(rays)
        path = tmp_path / "host.case"
        G.write_case(path, c["table"], before, g)
        host, _bits = G.host_step(hostgrating, path)
        assert np.array_equal(np.isnan(got), np.isnan(host))
        span = np.maximum(1.0, np.nanmax(np.abs(host), axis=1, keepdims=True))
        err = np.nan_to_num(np.abs(got - host) / span)
        print(f"{name}: device vs host {err.max():.3g}")
        assert err.max() <= DEVICE_VS_HOST, (name, err.max(axis=1))


@pytest.fixture(scope="module")
def big_reference(engines):
    """65 537 rays tiled from the 1027-ray sets, and their expected rows: computed once."""
    out = {}
    for name in G.BIG_CASES:
        c = G.case(name)
        m = c["big_in"].shape[1]
        idx = np.arange(65537) % m
        out[name] = (c["big_in"][:, idx], c["big_out"][:, idx])
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 65537])
@pytest.mark.parametrize("name", list(G.BIG_CASES))
def test_launch_sizes_check_every_lane(name, n, engines, big_reference):
    """The wave edge (63 / 64 / 65), several workgroups (257) and the launcher's switch from
    64-thread to 256-thread workgroups (65 536 rays and more): every lane, the NaN lanes of the
    evanescent case included."""
    c = G.case(name)
    g = c["g"]
    eng = engines(name)
    before, want = (a[:, :n] for a in big_reference[name])
    scale = G.scale_of(c["rows"])
    for dtype in (np.float64, np.float32):
        rays = _dev(before, dtype)
        status = eng.trace_grating(rays, g, 0, write_rays=True)
        assert status == _expect_status(want)
        got = _host(rays)
        G.compare(got, want, dtype, scale, f"{name} n={n}", report=print if n == 65537 else None)
        if dtype is np.float64:
            G.compare(got, want, dtype, scale, f"{name} n={n}", tight=True)
    if name.startswith("evan") and n >= 63:
        assert np.isnan(want[3]).any() and not np.isnan(want[3]).all()


def test_record_row_and_write_back(engines):
    """A record row inside a block whose stride is larger than n; write_rays with and without a
    record row; without write_rays the eight planes stay as they were."""
    name = "tilted"
    c = G.case(name)
    g = c["g"]
    eng = engines(name)
    before, want = c["rows"][g - 1], c["rows"][g]
    n = want.shape[1]
    scale = G.scale_of(c["rows"])
    block = torch.full((3, 8, n + 33), -7.0, dtype=torch.float64, device=DEV)
    rays = _dev(before)
    eng.trace_grating(rays, g, 0, record_row=block[1], write_rays=False)
    np.testing.assert_array_equal(_host(rays), before)               # not written
    got = block[1, :, :n].cpu().numpy()
    G.compare(got, want, np.float64, scale, "record row", tight=True)
    assert bool((block[0] == -7.0).all()) and bool((block[2] == -7.0).all()) \
        and bool((block[1, :, n:] == -7.0).all())
    eng.trace_grating(rays, g, 0, write_rays=True)                   # in place, no record row
    np.testing.assert_array_equal(_host(rays), got)
    rays = _dev(before)
    block.fill_(-7.0)
    eng.trace_grating(rays, g, 0, record_row=block[2], write_rays=True)
    np.testing.assert_array_equal(_host(rays), got)
    np.testing.assert_array_equal(block[2, :, :n].cpu().numpy(), got)
    with pytest.raises(ValueError, match="nothing to write"):
        eng.trace_grating(rays, g, 0, write_rays=False)
    with pytest.raises(ValueError, match="not a grating row"):
        eng.trace_grating(rays, g - 1, 0, write_rays=True)


def test_status_bit_of_an_evanescent_order():
    """OL_STATUS_NAN_DIRECTION when the grating is the LAST surface of the table, not with
    midrange; through `HipSystem.trace` too."""
    from optiland_amd.engine import HipSystem

    c = G.case("evan_m1")
    g = c["g"]
    full = c["table"]
    cut = S.SystemTable(surfaces=full.surfaces[:g + 1].copy(), coeffs=full.coeffs.copy(),
                        optics=full.optics[:g + 1].copy(), wavelengths=full.wavelengths.copy())
    eng = HipSystem(cut, DEV)
    try:
        assert eng.table.gratings == (g,) and eng.num_surfaces == g + 1
        for midrange, want in ((False, S.STATUS_NAN_DIRECTION), (True, 0)):
            rays = _dev(c["rows"][g - 1])
            assert eng.trace_grating(rays, g, 0, write_rays=True, midrange=midrange) == want
            got = _host(rays)
            nan = np.isnan(c["rows"][g][3])
            assert np.array_equal(np.isnan(got[3]), nan) and not np.isnan(got[:3]).any()
        res = eng.trace(_dev(c["rows"][0]), 0, record=True)
        assert res.status == S.STATUS_NAN_DIRECTION
        G.compare(res.record[:, :, :res.n].cpu().numpy(), c["rows"][:g + 1], np.float64,
                  G.scale_of(c["rows"]), "evan_m1 cut", tight=True)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(G.CASES))
def test_whole_optic_equals_the_fixture(name, engines):
    """`HipSystem.trace` over the whole table (fused run, grating, fused run) against the
    reference's `Optic.trace` records; the record block is one tensor."""
    c = G.case(name)
    eng = engines(name)
    n, last = c["rows"].shape[2], c["rows"].shape[0] - 1
    scale = G.scale_of(c["rows"])
    for dtype in (np.float64, np.float32):
        start = _dev(c["rows"][0], dtype)
        res = eng.trace(start, 0, record=True, first=0, last=last, check_status=True)
        assert isinstance(res.record, torch.Tensor) and res.record.shape[:2] == (last + 1, 8)
        got = res.record[:, :, :n].double().cpu().numpy()
        np.testing.assert_array_equal(_host(start), c["rows"][0].astype(dtype))   # not written
        G.compare(got, c["rows"], dtype, scale, name, report=print)
        if dtype is np.float64:
            G.compare(got, c["rows"], dtype, scale, name, tight=True, report=print)
        final = [t.clone() for t in start]
        eng.trace(final, 0, record=False, first=0, last=last)
        assert torch.equal(torch.stack(final).view(torch.uint8),
                           res.record[last, :, :n].contiguous().view(torch.uint8))


def test_c_entry_directly(engines):
    """OL_OK, the status word reads back, a wrong-kind surface gets its refusal text, a range
    entry refuses the grating row and launches nothing."""
    c = G.case("evan_p1")
    g = c["g"]
    eng = engines("evan_p1")
    lib, h = eng.lib, eng._handle
    before, want = c["rows"][g - 1], c["rows"][g]
    n = want.shape[1]
    rays_t = _dev(before)
    rays = (C.c_void_p * 8)(*[t.data_ptr() for t in rays_t])
    row = torch.full((8, n), -7.0, dtype=torch.float64, device=DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = eng._stream()
    with torch.cuda.device(eng.device):
        rc = lib.ol_trace_grating(h, _capi.F64, n, rays, 0, G.WAVELENGTH, row.data_ptr(), n, g, 0,
                                  word.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.ol_last_error()
        assert int(word.item()) == S.STATUS_NAN_DIRECTION
        G.compare(row.cpu().numpy(), want, np.float64, G.scale_of(c["rows"]), "C entry", tight=True)
        np.testing.assert_array_equal(_host(rays_t), before)          # no OL_TRACE_WRITE_RAYS
        rc = lib.ol_trace_grating(h, _capi.F64, n, rays, 0, G.WAVELENGTH, row.data_ptr(), n, g - 1,
                                  0, word.data_ptr(), stream)
        assert rc == -1 and lib.ol_last_error() == (
            b"ol_trace_grating: surface 2 is not a grating (geometry kind 0): trace it with "
            b"ol_trace")
        rc = lib.ol_trace_grating(h, _capi.F64, n, rays, 0, 0.0, row.data_ptr(), n, g, 0,
                                  word.data_ptr(), stream)
        assert rc == -1 and b"wavelength_um 0 must be finite and greater than 0" \
            in lib.ol_last_error()
        keep = row.clone()
        last = eng.num_surfaces - 1
        rc = lib.ol_trace(h, _capi.F64, n, rays, 0, None, 0, None, 0, last, 1, word.data_ptr(),
                          stream)
        assert rc == -2 and b"surface 3 is a diffraction grating" in lib.ol_last_error()
        torch.cuda.synchronize()
    assert torch.equal(row.view(torch.uint8), keep.view(torch.uint8))   # (NaN lanes: by bytes)
    np.testing.assert_array_equal(_host(rays_t), before)
    with pytest.raises(ValueError, match="gratings"):
        eng.trace(rays_t, 0, record=False, prt=torch.zeros((9, n), dtype=torch.float64, device=DEV))
