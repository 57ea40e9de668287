"""`ol_trace_opd_ensemble` / `SystemEnsemble.trace_opd` on the device:

* against the single launches: every fixture cell against `HipSystem(variant).wavefront_reference`
  + `trace_opd(reference=)`.  On-axis cells (field tangents exactly 0) are bit for bit the single
  launches -- the reference slot, OPD, intensity and the pupil planes.  Off axis the ensemble forms
  its tangents (and the launch-plane tilt) on the device and the single launch takes them from the
  host's libm, so the bound is MEASURED on the single launches themselves: they are run with `hy`
  moved one ulp each way, and four times the largest change seen is what the ensemble may differ
  by.  The moments are sums of the cell's own per-ray values in another order: the accumulation
  bound of tests/_exact_front.py (`opd_moment_bounds` with exact per-ray values) times `MARGIN`;
* against the reference fixture (tests/golden/ensemble_opd.npz, tests/_ensemble_opd.py) under the
  bounds of tests/test_ensemble_opd_cpu.py;
* shapes (1, 7, 257, 513 rays; one cell; 70 000 cells), planes on and off, the pupil flag, a
  padded stride, accumulation; `update`; a cell outside the ensemble; the refusals.
"""

import copy
import ctypes as C

import numpy as np
import pytest
import torch

from optiland_amd import _capi
from optiland_amd import system as S
from optiland_amd.analysis_seams import _launch_plane_tilt
from optiland_amd.engine import HipSystem
from optiland_amd.ensemble import (OPD_CELL_DTYPE, EnsembleWavefront, SystemEnsemble,
                                   opd_cell_grid, opd_statistics)
from tests import _ensemble as E
from tests import _ensemble_opd as EO
from tests import _exact_front as XF
from tests import _exact_trace as XT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SENTINEL = -7.25
_MEMO = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _ref_fields(r):
    """What a reference slot holds: its 15 doubles and the planar flag (the rest is padding)."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    return r[..., :15].tobytes() + r[..., 15:].view(np.int32)[..., :1].tobytes()


def launch(lens):
    """ONE ensemble call over every fixture cell of `lens`, pupil planes included (shared by the
    tests that read it): (tables, arrays, cells, moments (K, F, W, 12), refs (K, F, W, 16),
    planes (K, F, W, 5, N))."""
    if lens not in _MEMO:
        tabs, a = EO.tables(lens), EO.arrays(lens)
        K, F, W, n = a["opd"].shape
        cells = EO.cells(lens, tabs)
        ens = SystemEnsemble(tabs, DEV, F64)
        mom, refs, pb = ens.trace_opd(_t(a["px"]), _t(a["py"]), cells, planes=True, pupil=True)
        ens.close()
        _MEMO[lens] = (tabs, a, cells, mom.cpu().numpy().reshape(K, F, W, 12),
                       refs.cpu().numpy().reshape(K, F, W, 16),
                       pb[..., :n].cpu().numpy().reshape(K, F, W, 5, n))
    return _MEMO[lens]


def single(hs, table, field, wl, px, py):
    """The two single launches of one cell: (reference (16,), planes (5, n), moments (12,))."""
    rg = table.raygen
    hx, hy = float(field[0]), float(field[1])
    ux, uy = _launch_plane_tilt(rg, hx, hy)
    params = dict(n_image=rg["n_image"], ux=ux, uy=uy, half_epd=rg["EPD"] / 2.0,
                  wavelength_um=float(table.wavelengths[wl]),
                  last_thickness=float(table.last_thickness))
    ref, _chief = hs.wavefront_reference(params, wl, field=(hx, hy), pupil_z=rg["pupil_z"])
    opd, inten, pupil, mom = hs.trace_opd(None, px, py, wl, field=(hx, hy), want_pupil=True,
                                          reference=ref)
    return (ref.cpu().numpy(), torch.cat([opd[None], inten[None], pupil]).cpu().numpy(),
            mom.cpu().numpy())


@pytest.mark.parametrize("lens", E.LENSES)
def test_every_cell_is_the_single_launches_of_its_variant(lens):
    tabs, a, _cells, mom, refs, planes = launch(lens)
    px, py = _t(a["px"]), _t(a["py"])
    wls = EO.wavelength_indices(lens, tabs[0])
    keys = ("opd", "intensity", "pupil", "ref")
    moved = dict.fromkeys(keys, 0.0)    # the single launches, hy one ulp each way
    diff = dict.fromkeys(keys, 0.0)     # the ensemble against the single launches
    for k, t in enumerate(tabs):
        hs = HipSystem(t, DEV)
        for fi, (hx, hy) in enumerate(a["fields"]):
            for wi, w in enumerate(wls):
                ref, pl, m = single(hs, t, (hx, hy), w, px, py)
                got, lit = planes[k, fi, wi], planes[k, fi, wi, 1] > 0
                assert np.array_equal(lit, pl[1] > 0), (lens, k, fi, wi)
                assert mom[k, fi, wi, 9] == lit.sum() == m[9]
                if hx == 0.0 and hy == 0.0:
                    assert _ref_fields(refs[k, fi, wi]) == _ref_fields(ref), (lens, k, wi)
                    assert got.tobytes() == pl.tobytes(), (lens, k, wi)
                else:
                    for step in (np.inf, -np.inf):
                        r2, p2, _m = single(hs, t, (hx, np.nextafter(hy, step)), w, px, py)
                        assert np.array_equal(p2[1] > 0, lit)
                        moved["intensity"] = max(moved["intensity"],
                                                 float(np.abs(p2[1] - pl[1]).max()))
                        moved["opd"] = max(moved["opd"], float(np.abs(p2[0] - pl[0])[lit].max()))
                        moved["pupil"] = max(moved["pupil"],
                                             float(np.abs(p2[2:] - pl[2:])[:, lit].max()))
                        moved["ref"] = max(moved["ref"], float(np.abs(r2[:15] - ref[:15]).max()))
                    diff["opd"] = max(diff["opd"], float(np.abs(got[0] - pl[0])[lit].max()))
                    diff["intensity"] = max(diff["intensity"],
                                            float(np.abs(got[1] - pl[1]).max()))
                    diff["pupil"] = max(diff["pupil"],
                                        float(np.abs(got[2:] - pl[2:])[:, lit].max()))
                    diff["ref"] = max(diff["ref"],
                                      float(np.abs(refs[k, fi, wi, :15] - ref[:15]).max()))
                # the moments: sums of the cell's own per-ray values in another order
                inten, od, X, Y = got[1], got[0], got[2], got[3]
                want = np.array([inten.sum(), (inten * X).sum(), (inten * Y).sum(),
                                 (inten * X * X).sum(), (inten * X * Y).sum(),
                                 (inten * Y * Y).sum(), (inten * od).sum(),
                                 (inten * od * X).sum(), (inten * od * Y).sum(), lit.sum(),
                                 od[lit].sum(), (od[lit] ** 2).sum()])
                bound = XT.MARGIN * XF.opd_moment_bounds(inten, od, X, Y, lit, 0.0, 0.0, 0.0)
                err = np.abs(mom[k, fi, wi] - want)
                assert np.array_equal(np.isnan(want), np.isnan(mom[k, fi, wi]))
                ok = ~np.isnan(want)
                assert (err[ok] <= bound[ok]).all(), (lens, k, fi, wi, err, bound)
        hs.close()
    for key in moved:
        ratio = diff[key] / moved[key] if moved[key] else float("nan")
        print(f"[ensemble opd] {lens} {key}: ensemble against single launches {diff[key]:.3e}, "
              f"single launches under one ulp of hy {moved[key]:.3e}, ratio {ratio:.3f} (bound 4)")
    for key in moved:
        assert diff[key] <= 4.0 * moved[key], (lens, key, diff[key], moved[key])


@pytest.mark.parametrize("lens", E.LENSES)
def test_every_cell_against_the_reference_fixture(lens):
    tabs, a, _cells, mom, refs, planes = launch(lens)
    checks = EO.opd_checks(lens, planes[..., 0, :], planes[..., 1, :], a["opd"], a["intensity"])
    checks.append((f"{lens} radius (relative)",
                   float(np.abs(refs[..., 3] / a["radius"] - 1.0).max()), EO.RADIUS_RTOL))
    if lens == "cooke":
        assert mom[E.CLIPPED_VARIANT, 1, 0, 9] == EO.CLIPPED_KEPT and (mom[0, ..., 9] == 91).all()
    EO.report(checks)


@pytest.mark.parametrize("lens", E.LENSES)
def test_ensemble_wavefront_analysis(lens):
    """`EnsembleWavefront` -- its RMS, mean and radius from the device moments -- against the
    fixture's planes reduced in NumPy with `wavefront.OPD`'s definitions."""
    tabs, a = EO.tables(lens), EO.arrays(lens)
    ens = SystemEnsemble(tabs, DEV, F64)
    ew = EnsembleWavefront(ens, fields=a["fields"], wavelengths=a["wavelengths"],
                           num_rays=E.RINGS, maps=True)
    plain = EnsembleWavefront(ens, fields=a["fields"], wavelengths=a["wavelengths"],
                              num_rays=E.RINGS)
    ens.close()
    assert plain.opd is None and plain.intensity is None
    assert np.array_equal(plain.moments[..., 9:], ew.moments[..., 9:])
    assert ew.opd.shape == a["opd"].shape == ew.intensity.shape
    lit = a["intensity"] > 0
    o = np.where(lit, a["opd"], 0.0)
    rms = np.sqrt((o * o).sum(-1) / lit.sum(-1))
    mean = o.sum(-1) / lit.sum(-1)
    scale = max(1.0, float(np.abs(a["opd"][lit]).max()))
    checks = EO.opd_checks(lens, ew.opd, ew.intensity, a["opd"], a["intensity"])
    checks += [(f"{lens} rms [waves]", float(np.abs(ew.rms() - rms).max()),
                EO.OPD_BOUND[lens] * scale),
               (f"{lens} mean [waves]", float(np.abs(ew.mean() - mean).max()),
                EO.OPD_BOUND[lens] * scale),
               (f"{lens} radius (relative)", float(np.abs(ew.radius / a["radius"] - 1.0).max()),
                EO.RADIUS_RTOL)]
    EO.report(checks)
    assert np.array_equal(ew.rms(), opd_statistics(ew.moments)[0])


# ------------------------------------------------------------------ shapes
def _points(n):
    rng = np.random.default_rng(n)
    r, th = np.sqrt(rng.random(n)) * 0.95, rng.random(n) * 2 * np.pi
    x, y = r * np.cos(th), r * np.sin(th)
    x[0] = y[0] = 0.0
    return x, y


@pytest.mark.parametrize("n", [1, 7, 257, 513])
def test_ray_counts_around_a_workgroup(n):
    """One ray, a few, one lane past a workgroup of 256 and one past two: the on-axis cells are
    the single launches bit for bit, every cell counts its rays, and `planes=None` gives the
    same moments and references."""
    tabs = EO.tables("singlet")[:3]
    x, y = _points(n)
    px, py = _t(x), _t(y)
    cells = opd_cell_grid(tabs, [(0.0, 0.0), (0.0, 1.0)], [0, 1])
    ens = SystemEnsemble(tabs, DEV, F64)
    mom, refs, pb = ens.trace_opd(px, py, cells, planes=True, pupil=True)
    mom0, refs0, none = ens.trace_opd(px, py, cells)
    ens.close()
    assert none is None and pb.shape == (12, 5, n)
    assert torch.equal(mom, mom0) or np.allclose(mom.cpu(), mom0.cpu(), rtol=1e-12, atol=1e-12)
    assert _ref_fields(refs.cpu().numpy()) == _ref_fields(refs0.cpu().numpy())
    mom, pb, refs = mom.cpu().numpy(), pb.cpu().numpy(), refs.cpu().numpy()
    assert (mom[:, 9] == (pb[:, 1] > 0).sum(-1)).all() and (mom[:, 9] > 0).all()
    for k, t in enumerate(tabs):
        hs = HipSystem(t, DEV)
        for wi in (0, 1):
            ref, pl, _m = single(hs, t, (0.0, 0.0), wi, px, py)
            c = (k * 2 + 0) * 2 + wi
            assert pb[c].tobytes() == pl.tobytes() and _ref_fields(refs[c]) == _ref_fields(ref)
        hs.close()


def test_one_cell():
    tabs, a = EO.tables("cooke"), EO.arrays("cooke")
    cells = EO.cells("cooke", tabs)
    ens = SystemEnsemble(tabs, DEV, F64)
    mom, refs, pb = ens.trace_opd(_t(a["px"]), _t(a["py"]), cells[3, 1, 0], planes=True,
                                  pupil=True)
    ens.close()
    _tabs, _a, _c, m, r, p = launch("cooke")
    assert mom.shape == (1, 12) and refs.shape == (1, 16) and pb.shape == (1, 5, 91)
    assert pb[0].cpu().numpy().tobytes() == p[3, 1, 0].tobytes()
    assert _ref_fields(refs[0].cpu().numpy()) == _ref_fields(r[3, 1, 0])
    assert mom[0, 9] == EO.CLIPPED_KEPT


def test_seventy_thousand_cells():
    """More cells than a grid dimension holds (65535): 70 000 cells of one ray over K = 3.  Each
    cell equals its neighbour of the same variant, field and wavelength."""
    tabs = EO.tables("cooke")[:3]
    px, py = _t([0.3]), _t([-0.4])
    base = opd_cell_grid(tabs, [(0.0, 0.0), (0.0, 0.7), (0.5, 0.5)], [0, 1]).reshape(-1)  # 18
    cells = np.resize(base, 70000)
    ens = SystemEnsemble(tabs, DEV, F64)
    mom, refs, pb = ens.trace_opd(px, py, cells, planes=True, pupil=True)
    small, rs, ps = ens.trace_opd(px, py, base, planes=True, pupil=True)
    ens.close()
    reps = np.resize(np.arange(18), 70000)
    assert (mom[:, 9] == 1).all()
    assert np.array_equal(mom.cpu().numpy(), small.cpu().numpy()[reps])
    assert np.array_equal(pb.cpu().numpy(), ps.cpu().numpy()[reps])
    assert _ref_fields(refs.cpu().numpy()) == _ref_fields(rs.cpu().numpy()[reps])


@pytest.mark.parametrize("pupil", [False, True])
def test_a_padded_stride_is_left_alone_and_moments_accumulate(pupil):
    tabs, a = EO.tables("cooke")[:2], EO.arrays("cooke")
    px, py, n = _t(a["px"]), _t(a["py"]), 91
    cells = opd_cell_grid(tabs, [(0.0, 0.7)], [0, 1])
    P, stride = (5 if pupil else 2), n + 13
    block = torch.full((4, P, stride), SENTINEL, dtype=F64, device=DEV)
    ens = SystemEnsemble(tabs, DEV, F64)
    mom, _r, pb = ens.trace_opd(px, py, cells, planes=block, pupil=pupil)
    tight, _r2, pt = ens.trace_opd(px, py, cells, planes=True, pupil=pupil)
    again, _r3, _p = ens.trace_opd(px, py, cells, out=mom.clone())
    ens.close()
    assert pb is block and (block[..., n:] == SENTINEL).all()
    assert torch.equal(block[..., :n], pt[..., :n]) and not (block[..., :n] == SENTINEL).any()
    assert torch.equal(mom, tight)
    assert torch.equal(again, 2 * mom)          # (x + x is exact)
    _t2, _a, _c, _m, _refs, p = launch("cooke")
    assert block[:, :P, :n].cpu().numpy().tobytes() == p[:2, 1, :, :P].tobytes()


# ------------------------------------------------------------------ update, bad cells, refusals
def test_update_rewrites_one_variant_only():
    tabs, a = EO.tables("cooke"), EO.arrays("cooke")
    px, py = _t(a["px"]), _t(a["py"])
    start = [tabs[0], tabs[0], tabs[0]]
    ens = SystemEnsemble(start, DEV, F64)
    cells = opd_cell_grid(start, a["fields"], [0, 1])
    m0, r0, p0 = ens.trace_opd(px, py, cells, planes=True, pupil=True)
    ens.update(1, tabs[EO.THICKNESS_VARIANT])
    cells = opd_cell_grid(ens.tables, a["fields"], [0, 1])     # (the variant's own exit pupil)
    m1, r1, p1 = ens.trace_opd(px, py, cells, planes=True, pupil=True)
    ens.close()
    _t2, _a, _c, m, r, p = launch("cooke")
    p0, p1 = (v.cpu().numpy().reshape(3, -1) for v in (p0, p1))
    m0, m1 = (v.cpu().numpy().reshape(3, -1) for v in (m0, m1))
    r0, r1 = (v.cpu().numpy().reshape(3, 4, 16) for v in (r0, r1))
    for k in (0, 2):
        assert p1[k].tobytes() == p0[k].tobytes() and m1[k].tobytes() == m0[k].tobytes()
        assert _ref_fields(r1[k]) == _ref_fields(r0[k])
    assert p1[1].tobytes() != p0[1].tobytes()
    assert p1[1].tobytes() == p[EO.THICKNESS_VARIANT].tobytes()
    assert _ref_fields(r1[1]) == _ref_fields(r[EO.THICKNESS_VARIANT].reshape(4, 16))


@pytest.mark.parametrize("what", ["variant", "wavelength_index"])
def test_a_cell_outside_the_ensemble_is_skipped_and_reported(what):
    tabs, a = EO.tables("cooke")[:2], EO.arrays("cooke")
    px, py, n = _t(a["px"]), _t(a["py"]), 91
    cells = opd_cell_grid(tabs, [(0.0, 0.7)], [0, 1]).reshape(-1).copy()      # 4 cells
    good = cells.copy()
    cells[what][1] = 2 if what == "variant" else -1
    ens = SystemEnsemble(tabs, DEV, F64)
    with pytest.raises(IndexError, match="does not hold"):
        ens.trace_opd(px, py, cells)

    def run(c):
        out = (torch.full((4, 12), SENTINEL, dtype=F64, device=DEV),
               torch.full((4, 16), SENTINEL, dtype=F64, device=DEV),
               torch.full((4, 5, n), SENTINEL, dtype=F64, device=DEV))
        ens.trace_opd(px, py, c, planes=out[2], pupil=True, out=out[0], refs=out[1],
                      check_status=False)
        return [v.cpu().numpy() for v in out]

    mom, refs, pb = run(cells)
    status = int(ens._status.item())
    want = run(good)
    ens.close()
    assert status == _capi.STATUS_ENSEMBLE_CELL
    assert (mom[1] == SENTINEL).all() and (refs[1] == SENTINEL).all() and (pb[1] == SENTINEL).all()
    for c in (0, 2, 3):
        assert pb[c].tobytes() == want[2][c].tobytes() and mom[c].tobytes() == want[0][c].tobytes()
        assert _ref_fields(refs[c]) == _ref_fields(want[1][c])


def test_refusals_launch_nothing():
    lib = _capi.load()
    tabs, a = EO.tables("cooke")[:2], EO.arrays("cooke")
    px, py, n = _t(a["px"]), _t(a["py"]), 91
    host = np.ascontiguousarray(opd_cell_grid(tabs, [(0.0, 0.7)], [0]).reshape(-1))
    cells = torch.from_numpy(host.view(np.uint8)).to(DEV)
    assert host.dtype == OPD_CELL_DTYPE
    mom = torch.full((2, 12), SENTINEL, dtype=F64, device=DEV)
    refs = torch.full((2, 16), SENTINEL, dtype=F64, device=DEV)
    pb = torch.full((2, 2, n), SENTINEL, dtype=F64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    inp = _capi.RaygenInputs(None, None, px.data_ptr(), py.data_ptr(), None, None, 0.0, 0.0, 1.0,
                             1.0, 0, 0)

    def call(ens, dt=_capi.F64, stride=n, st=status):
        rc = lib.ol_trace_opd_ensemble(ens._handle, dt, n, C.byref(inp), 2, cells.data_ptr(),
                                       refs.data_ptr(), pb.data_ptr(), stride, mom.data_ptr(),
                                       st.data_ptr() if st is not None else None, None)
        torch.cuda.synchronize()
        return rc, lib.ol_last_error().decode()

    def untouched():
        return bool((mom == SENTINEL).all() and (refs == SENTINEL).all()
                    and (pb == SENTINEL).all() and int(status.item()) == 0)

    ens = SystemEnsemble(tabs, DEV, F64)
    rc, msg = call(ens, dt=_capi.F32)
    assert rc == -2 and "fp64 only" in msg and untouched()
    rc, msg = call(ens, st=None)
    assert rc == -1 and "NULL argument" in msg and untouched()
    rc, msg = call(ens, stride=n - 1)
    assert rc == -1 and "planes_stride 90 < 91 rays" in msg and untouched()
    with pytest.raises(ValueError, match="fp64 only"):
        SystemEnsemble(tabs, DEV, torch.float32).trace_opd(px.float(), py.float(), host)
    # polarisation-dependent coatings, as ol_trace_opd
    coated = [copy.deepcopy(t) for t in tabs]
    for t in coated:
        t.surfaces["coating_kind"][2] = S.COAT_FRESNEL
    pol = SystemEnsemble(coated, DEV, F64)
    rc, msg = call(pol)
    pol.close()
    assert rc == -1 and "Polarization must be set" in msg and untouched()
    # ... and the same call, unrefused, writes all three
    rc, msg = call(ens)
    ens.close()
    assert rc == 0, msg
    assert not (mom[:, 9] == SENTINEL).any() and not (refs[:, :15] == SENTINEL).any()
    assert not (pb == SENTINEL).any()
