"""`ol_trace_spot_ensemble` on the device: K variants of one optic in ONE launch.

* against single launches: every fixture cell's hits are those of `HipSystem.trace_spot` on a
  system built from that variant alone, bit for bit, in fp32 and fp64.  The ensemble forms a
  cell's field tangents on the device from the VARIANT's constants -- the arithmetic of per-ray
  field planes -- so the single launch it is held against is the field-plane form (the
  launch-uniform form takes its tangents from the host's libm).  The moments are sums of the same
  terms in another order: bounded by the accumulation bound of tests/_exact_front.py
  (`spot_bounds` with exact hits: n eps sum |term|), times `MARGIN` = 2 for the two orderings;
* against the reference fixture (tests/golden/ensemble.npz, tests/_ensemble.py): hits and the
  `rms_spot_size` operand to the project's contracts;
* the ray-generation constants are per variant; shapes (one ray, a ragged tail, 70 000 cells);
  `update` rewrites one variant only; refusals launch nothing.
"""

import copy

import numpy as np
import pytest
import torch

from optiland_amd import _capi
from optiland_amd import system as S
from optiland_amd.engine import HipSystem
from optiland_amd.ensemble import (StructureMismatch, SystemEnsemble, UnsupportedStructure,
                                   cell_grid, rms_about_centroid)
from tests import _ensemble as E
from tests import _exact_front as XF
from tests import _exact_trace as XT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f64": torch.float64}
_MEMO = {}


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV, dtype)


def launch(lens, tag):
    """ONE ensemble launch over every fixture cell of `lens` (shared by the tests that read it):
    (tables, arrays, hits (K, F, W, 3, N) in the dtype, moments (K, F, W, 8), centres (F, 2))."""
    key = (lens, tag)
    if key not in _MEMO:
        tabs, a = E.tables(lens), E.arrays(lens)
        dt = DTYPES[tag]
        ens = SystemEnsemble(tabs, DEV, dt)
        assert ens.size == len(tabs) == 6
        K, F, W = a["hits"].shape[:3]
        centers = a["hits"][0, :, 0, :2, 0]          # the nominal chief-ray hits (point 0: axis)
        cells = cell_grid(K, a["fields"], E.wavelength_indices(lens, tabs[0]), centers=centers)
        mom, hb = ens.trace_spot(_t(a["px"], dt), _t(a["py"], dt), cells, hits=True)
        n = a["px"].size
        _MEMO[key] = (tabs, a, hb[..., :n].cpu().numpy().reshape(K, F, W, 3, n),
                      mom.cpu().numpy().reshape(K, F, W, 8), centers)
        ens.close()
    return _MEMO[key]


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("lens", E.LENSES)
def test_every_cell_is_the_single_launch_of_its_variant(lens, tag):
    tabs, a, hits, mom, centers = launch(lens, tag)
    dt, n = DTYPES[tag], a["px"].size
    px, py = _t(a["px"], dt), _t(a["py"], dt)
    wls = E.wavelength_indices(lens, tabs[0])
    worst = 0.0
    for k, t in enumerate(tabs):
        hs = HipSystem(t, DEV)
        for fi, (hx, hy) in enumerate(a["fields"]):
            fx = torch.full((n,), float(hx), dtype=dt, device=DEV)
            fy = torch.full((n,), float(hy), dtype=dt, device=DEV)
            for wi, w in enumerate(wls):
                planes = [torch.empty(n, dtype=dt, device=DEV) for _ in range(3)]
                m = hs.trace_spot(px, py, w, hx=fx, hy=fy, center=tuple(centers[fi]),
                                  hits=planes).cpu().numpy()
                single = torch.stack(planes).cpu().numpy()
                got = hits[k, fi, wi]
                assert got.tobytes() == single.tobytes(), (lens, tag, k, fi, wi)
                x, y, i = got.astype(np.float64)
                lit = i > 0
                bound = XT.MARGIN * XF.spot_bounds(x, y, i, lit, centers[fi][0], centers[fi][1],
                                                   0.0, 0.0, "f64")
                err = np.abs(mom[k, fi, wi, :7] - m)
                print(lens, tag, "variant", k, "field", fi, "wl", wi, "moment err", err.tolist(),
                      "bound", bound.tolist())
                assert (err <= bound).all(), (lens, tag, k, fi, wi, err, bound)
                assert mom[k, fi, wi, 0] == lit.sum() and mom[k, fi, wi, 7] == 0.0
                worst = max(worst, float(err.max()))
        hs.close()
    print(lens, tag, "largest moment difference", worst)


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("lens", E.LENSES)
def test_every_cell_against_the_reference_fixture(lens, tag):
    tabs, a, hits, mom, centers = launch(lens, tag)
    want = a["hits"]
    tol = E.contract(lens, 32 if tag == "f32" else 64)
    scale = float(np.abs(want[:, :, :, :2]).max())
    lit = want[:, :, :, 2] > 0
    assert np.array_equal(hits[:, :, :, 2] > 0, lit)
    assert (lit.sum(axis=-1)[E.CLIPPED_VARIANT] < E.N_RAYS).any() or lens != "cooke"
    err = np.abs(hits[:, :, :, :2].astype(np.float64) - want[:, :, :, :2])
    print(lens, tag, "hits: max |err| / scale", err.max() / scale, "contract", tol)
    assert err.max() <= tol * scale
    assert np.abs(hits[:, :, :, 2] - want[:, :, :, 2]).max() <= tol
    # the operand: an unmasked mean over all rays.  Where no ray was lost it follows from the
    # device moments (about the centroid), elsewhere from the cell's hits as the operand does
    full = mom[..., 0] == a["px"].size
    from_moments = rms_about_centroid(mom)
    from_hits = np.array([[[E.operand_from_hits(*hits[k, f, w, :2].astype(np.float64))
                            for w in range(hits.shape[2])] for f in range(hits.shape[1])]
                          for k in range(hits.shape[0])])
    got = np.where(full, from_moments, from_hits)
    oerr = np.abs(got - a["operand"])
    print(lens, tag, "operand: max |err| / scale", oerr.max() / scale, "cells from moments",
          int(full.sum()), "of", full.size)
    assert oerr.max() <= tol * scale
    if lens == "cooke":
        assert not full[E.CLIPPED_VARIANT].all() and full[0].all()


@pytest.mark.parametrize("lens", E.LENSES)
def test_the_ray_generation_constants_are_per_variant(lens):
    """The radius in front of the stop moves the entrance pupil: traced with variant 0's
    ray-generation constants the variant's rays are other rays."""
    tabs, a, hits, _mom, centers = launch(lens, "f64")
    k = E.RADIUS_VARIANT
    assert tabs[k].raygen["EPL"] != tabs[0].raygen["EPL"]
    shared = [copy.deepcopy(t) for t in tabs]
    shared[k].raygen = dict(tabs[0].raygen)
    ens = SystemEnsemble(shared, DEV, torch.float64)
    cells = cell_grid(len(tabs), a["fields"], E.wavelength_indices(lens, tabs[0]), centers=centers)
    _m, hb = ens.trace_spot(_t(a["px"], torch.float64), _t(a["py"], torch.float64), cells,
                            hits=True)
    ens.close()
    wrong = hb[..., :a["px"].size].cpu().numpy().reshape(hits.shape)
    tol = E.contract(lens, 64) * float(np.abs(a["hits"][:, :, :, :2]).max())
    assert wrong[k, 1].tobytes() != hits[k, 1].tobytes()               # the off-axis field
    off = np.abs(wrong[k, 1, :, :2] - a["hits"][k, 1, :, :2]).max()
    print(lens, "hits with variant 0's constants: max |err|", off, "contract", tol)
    if lens == "cooke":   # (1e-12 of the image height: the shared constants miss it by far)
        assert off > 100 * tol, off
    assert np.abs(hits[k, :, :, :2] - a["hits"][k, :, :, :2]).max() <= tol
    others = [j for j in range(len(tabs)) if j != k]
    assert wrong[others].tobytes() == hits[others].tobytes()


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 91, 1025, 1027, 2051])
def test_ray_counts_around_a_tile(n, tag):
    """One ray, the fixture's 91, and counts just past one tile of the vector forms (256 lanes x 4
    fp32 rays = 1024, x 2 fp64 rays = 512: 1025 ... 2051 leave ragged tails of 1 and 3 rays) and
    past one tile of the one-ray forms: every cell equals its variant's single launch."""
    dt = DTYPES[tag]
    tabs = E.tables("cooke")[:3]
    rng = np.random.default_rng(n)
    r, th = np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    px, py = _t(r * np.cos(th), dt), _t(r * np.sin(th), dt)
    fields = [(0.0, 0.0), (0.3, -0.6)]
    ens = SystemEnsemble(tabs, DEV, dt)
    mom, hb = ens.trace_spot(px, py, cell_grid(3, fields, [0, 1]), hits=True)
    ens.close()
    hb = hb[..., :n].cpu().numpy().reshape(3, 2, 2, 3, n)
    mom = mom.cpu().numpy().reshape(3, 2, 2, 8)
    for k, t in enumerate(tabs):
        hs = HipSystem(t, DEV)
        for fi, (hx, hy) in enumerate(fields):
            fx = torch.full((n,), hx, dtype=dt, device=DEV)
            fy = torch.full((n,), hy, dtype=dt, device=DEV)
            for w in (0, 1):
                planes = [torch.empty(n, dtype=dt, device=DEV) for _ in range(3)]
                m = hs.trace_spot(px, py, w, hx=fx, hy=fy, hits=planes).cpu().numpy()
                assert hb[k, fi, w].tobytes() == torch.stack(planes).cpu().numpy().tobytes()
                assert mom[k, fi, w, 0] == m[0]
        hs.close()


def test_seventy_thousand_cells():
    """More cells than a grid dimension holds (65535): 70 000 cells of 7 rays over K = 3."""
    dt = torch.float32
    tabs = E.tables("cooke")[:3]
    x, y = np.array([0.0, 1, 0.5, -0.5, -1, -0.5, 0.5]), np.array([0.0, 0, 0.8, 0.8, 0, -0.8, -0.8])
    base = cell_grid(3, [(0.0, 0.0), (0.0, 0.7), (0.5, 0.5)], [0, 1]).reshape(-1)   # 18 cells
    cells = np.resize(base, 70000)
    ens = SystemEnsemble(tabs, DEV, dt)
    mom, hb = ens.trace_spot(_t(x, dt), _t(y, dt), cells, hits=True)
    small, hs = ens.trace_spot(_t(x, dt), _t(y, dt), base, hits=True)
    ens.close()
    mom, small = mom.cpu().numpy(), small.cpu().numpy()
    assert (mom[:, 0] == 7).all()
    reps = np.resize(np.arange(18), 70000)
    assert np.array_equal(mom, small[reps])
    hb, hs = hb[..., :7].cpu().numpy(), hs[..., :7].cpu().numpy()
    assert np.array_equal(hb, hs[reps])


def test_update_rewrites_one_variant_only():
    dt = torch.float64
    tabs, a = E.tables("cooke"), E.arrays("cooke")
    start = [tabs[0], tabs[0], tabs[0]]
    cells = cell_grid(3, a["fields"], [0, 1])
    px, py = _t(a["px"], dt), _t(a["py"], dt)
    ens = SystemEnsemble(start, DEV, dt)
    m0, h0 = ens.trace_spot(px, py, cells, hits=True)
    ens.update(1, tabs[E.RADIUS_VARIANT])
    m1, h1 = ens.trace_spot(px, py, cells, hits=True)
    want = SystemEnsemble([tabs[0], tabs[E.RADIUS_VARIANT], tabs[0]], DEV, dt)
    m2, h2 = want.trace_spot(px, py, cells, hits=True)
    ens.close()
    want.close()
    n = a["px"].size          # (the planes are padded to 16 bytes: the padding is never written)
    h0, h1, h2 = (h[..., :n].cpu().numpy().reshape(3, -1) for h in (h0, h1, h2))
    assert h1[0].tobytes() == h0[0].tobytes() and h1[2].tobytes() == h0[2].tobytes()
    assert h1[1].tobytes() != h0[1].tobytes()
    assert h1.tobytes() == h2.tobytes()
    assert np.array_equal(m1.cpu().numpy(), m2.cpu().numpy())


def test_a_cell_outside_the_ensemble_is_skipped_and_reported():
    dt = torch.float64
    tabs = E.tables("cooke")[:2]
    ens = SystemEnsemble(tabs, DEV, dt)
    cells = cell_grid(2, [(0.0, 0.0)], [0]).reshape(-1).copy()
    cells["variant"][1] = 2
    z = torch.zeros(1, dtype=dt, device=DEV)
    with pytest.raises(IndexError, match="does not hold"):
        ens.trace_spot(z, z, cells)
    mom, _ = ens.trace_spot(z, z, cells, check_status=False)
    ens.close()
    assert mom.cpu().numpy()[:, 0].tolist() == [1.0, 0.0]


def test_refusals_launch_nothing():
    tabs = E.tables("cooke")
    lib = _capi.load()
    # a structure mismatch: on the host first, and by the library when the host check is passed by
    bad = copy.deepcopy(tabs[1])
    bad.surfaces["aperture_kind"][3] = S.AP_RADIAL
    with pytest.raises(StructureMismatch, match="variant 1, surface 3: aperture_kind"):
        SystemEnsemble([tabs[0], bad], DEV)
    recs, keep = SystemEnsemble._records([tabs[0], bad])
    import ctypes as C
    handle = C.c_void_p()
    rc = lib.ol_ensemble_create(recs, 2, tabs[0].num_surfaces, tabs[0].optics.shape[1],
                                C.byref(handle))
    assert rc == -1 and handle.value is None
    assert b"variant 1, surface 3: aperture_kind 1 differs from variant 0's 0" in lib.ol_last_error()
    # a one-launch kind and a reference-rule Newton surface
    forbes = copy.deepcopy(tabs[0])
    forbes.surfaces["geom_kind"][2] = S.GEOM_FORBES_Q
    forbes.__dict__.pop("_single_rows", None)
    with pytest.raises(UnsupportedStructure, match="surface 2 is a Forbes surface"):
        SystemEnsemble([forbes], DEV)
    newton = E.tables("singlet")[0]
    newton.surfaces["flags"][1] |= S.SURF_REFERENCE_NEWTON
    with pytest.raises(UnsupportedStructure, match="OL_SURF_REFERENCE_NEWTON"):
        SystemEnsemble([newton], DEV)
    recs, keep = SystemEnsemble._records([newton])
    rc = lib.ol_ensemble_create(recs, 1, newton.num_surfaces, newton.optics.shape[1],
                                C.byref(handle))
    assert rc == -2 and handle.value is None and b"OL_SURF_REFERENCE_NEWTON" in lib.ol_last_error()
    # an update that breaks the structure changes nothing
    ens = SystemEnsemble(tabs[:2], DEV, torch.float64)
    z = torch.zeros(1, dtype=torch.float64, device=DEV)
    cells = cell_grid(2, [(0.0, 0.7)], [0])
    _m, before = ens.trace_spot(z, z, cells, hits=True)
    with pytest.raises(StructureMismatch, match="variant 1, surface 3"):
        ens.update(1, bad)
    recs, keep = SystemEnsemble._records([bad])
    rc = lib.ol_ensemble_update(ens._handle, 1, 1, recs, None)
    assert rc == -1 and b"variant 1, surface 3" in lib.ol_last_error()
    _m, after = ens.trace_spot(z, z, cells, hits=True)
    assert before[..., :1].cpu().numpy().tobytes() == after[..., :1].cpu().numpy().tobytes()
    ens.close()


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_three_variants_against_the_exact_trace(tag):
    """Three Cooke variants x one field against `_exact_front.gen_ray` + `_exact_trace.trace_ray`
    at 50 digits, under `_exact_trace.bound` (tests/_ensemble.py: exact_case): the one check that
    is not held against another kernel of this project."""
    dt = DTYPES[tag]
    px, py, hx, hy = E.exact_inputs()
    ens = SystemEnsemble(E.tables("cooke"), DEV, dt)
    cells = np.concatenate([cell_grid(6, [(hx, hy)], [E.EXACT_WL]).reshape(-1)[[k]]
                            for k in E.EXACT_VARIANTS])
    _m, hb = ens.trace_spot(_t(px, dt), _t(py, dt), cells, hits=True)
    ens.close()
    hb = hb[..., :px.size].double().cpu().numpy()
    checks = E.exact_checks({k: hb[i] for i, k in enumerate(E.EXACT_VARIANTS)}, tag)
    for label, err, bound in checks:
        print(f"[exact ensemble] {tag} {label:60s} {err:.3e} / {bound:.3e}")
    assert not [(lab, e, b) for lab, e, b in checks if not e <= b]


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_ensemble_spot_analysis(tag):
    """`EnsembleSpot` with its defaults -- fields="all", wavelengths="all", the centres from the
    nominal variant's chief rays at the reference wavelength -- against the fixture's hits
    reduced in NumPy with `SpotDiagram`'s definitions, for every variant, and against
    `analysis.SpotDiagram` itself on a tracer of the nominal variant."""
    from optiland_amd.analysis import SpotDiagram
    from optiland_amd.ensemble import EnsembleSpot
    from optiland_amd.tracer import HipRayTracer
    tabs, a = E.tables("cooke"), E.arrays("cooke")
    dt = DTYPES[tag]
    ens = SystemEnsemble(tabs, DEV, dt)
    es = EnsembleSpot(ens, num_rays=E.RINGS)
    ens.close()
    K, W = len(tabs), len(a["wavelengths"])
    assert es.moments.shape == (K, 3, W, 8) and es.num_points == E.N_RAYS   # 3 fields in the table
    assert es.fields[:2] == [tuple(f) for f in a["fields"]] and es.fields[2] == (0.0, 1.0)
    assert es.wavelengths == list(a["wavelengths"]) and es.ref_index == 1   # 0.55 um is primary
    want = a["hits"]                                                        # (K, 2, W, 3, N)
    tol = E.contract("cooke", 32 if tag == "f32" else 64) * float(np.abs(want[:, :, :, :2]).max())
    # the default centres: the nominal chief rays AT THE REFERENCE WAVELENGTH (pupil point 0)
    assert np.abs(es.centers[:2] - want[0, :, es.ref_index, :2, 0]).max() <= tol
    lit = want[:, :, :, 2] > 0
    n = lit.sum(-1)
    x, y = want[:, :, :, 0], want[:, :, :, 1]
    cx, cy = (es.centers[None, :2, None, i, None] for i in (0, 1))
    centroid = np.stack([(x * lit).sum(-1) / n, (y * lit).sum(-1) / n], axis=-1)
    r2 = ((x - cx) ** 2 + (y - cy) ** 2) * lit
    assert np.abs(es.centroid()[:, :2] - centroid).max() <= tol
    assert np.abs(es.rms_spot_radius()[:, :2] - np.sqrt(r2.sum(-1) / n)).max() <= 2 * tol
    assert np.abs(es.geometric_spot_radius()[:, :2] - np.sqrt(r2.max(-1))).max() <= 2 * tol
    assert (es.moments[:, :2, :, 0] == n).all()
    own = np.sqrt((((x - centroid[..., 0, None]) ** 2 + (y - centroid[..., 1, None]) ** 2)
                   * lit).sum(-1) / n)
    assert np.abs(es.rms_about_centroid()[:, :2] - own).max() <= 2 * tol
    # ... and the project's own single-system analysis of the nominal variant
    sd = SpotDiagram(HipRayTracer(tabs[0], DEV, dtype=dt), num_rings=E.RINGS,
                     coordinates="global")
    assert np.abs(np.array(sd.centroid()) - es.centroid()[0, :, es.ref_index]).max() <= tol
    assert np.abs(np.array(sd.rms_spot_radius()) - es.rms_spot_radius()[0]).max() <= 2 * tol
    assert np.abs(np.array(sd.geometric_spot_radius())
                  - es.geometric_spot_radius()[0]).max() <= 2 * tol
