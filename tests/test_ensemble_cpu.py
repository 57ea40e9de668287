"""The ensemble (K variants of one optic per launch) without a GPU: the structure check and its
texts (Python and C alike), the moment -> radius arithmetic against `analysis.SpotDiagram`'s, the
cell ordering, `pack_ensemble`, and the cell walk of csrc/ensemble_device.h run on the CPU by the
stand-alone program tests/hostensemble -- bit for bit the host run of each variant alone, and
within the project's contracts of the reference fixture tests/golden/ensemble.npz
(tests/_ensemble.py).  No GPU needed."""

import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from optiland_amd import _capi, analysis, build
from optiland_amd import system as S
from optiland_amd.ensemble import (CELL_DTYPE, STRUCTURE_FIELDS, StructureMismatch,
                                   SystemEnsemble, UnsupportedStructure, cell_grid,
                                   check_structure, radii_from_moments, rms_about_centroid)
from tests import _ensemble as E
from tests import _live

host = pytest.mark.skipif(not E._builder().available(), reason="needs hipcc (host compile)")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _capi.load()


# ------------------------------------------------------------------ structure
def _break(table, field):
    bad = copy.deepcopy(table)
    s = bad.surfaces
    if field == "geom_kind":
        s["geom_kind"][2] = S.GEOM_PLANE
    elif field == "n_coeff":
        s["n_coeff"][1] += 1
    elif field == "aperture_kind":
        s["aperture_kind"][3] = S.AP_RADIAL
    elif field == "flags":
        s["flags"][2] |= S.SURF_REFERENCE_ROOT
    elif field == "interaction":
        s["interaction"][2] = S.INTERACT_REFLECT
    elif field == "coating_kind":
        s["coating_kind"][2] = S.COAT_SIMPLE
    return bad


SURFACE_OF = {"geom_kind": 2, "n_coeff": 1, "aperture_kind": 3, "flags": 2, "interaction": 2,
              "coating_kind": 2}


def _c_create(lib, tables):
    recs, keep = SystemEnsemble._records(tables)
    handle = C.c_void_p()
    rc = lib.ol_ensemble_create(recs, len(tables), tables[0].num_surfaces,
                                tables[0].optics.shape[1], C.byref(handle))
    del keep
    msg = lib.ol_last_error().decode()
    if rc == 0:     # (a machine with a GPU: the ensemble exists, and goes again)
        lib.ol_ensemble_destroy(handle)
        handle = C.c_void_p()
    return rc, msg, handle


@pytest.mark.parametrize("field", sorted(SURFACE_OF))
def test_a_variant_that_differs_in_structure_is_named(lib, field):
    """One case per differing field: the variant, the surface and the field, in the same words
    from the Python check and from the library (which refuses before it asks for a device)."""
    tabs = E.tables("singlet" if field == "n_coeff" else "cooke")
    bad = _break(tabs[2], field)
    with pytest.raises(StructureMismatch) as exc:
        check_structure([tabs[0], tabs[1], bad])
    text = str(exc.value)
    assert re.match(rf"ol_ensemble_create: variant 2, surface {SURFACE_OF[field]}: {field} -?\d+ "
                    rf"differs from variant 0's -?\d+ \(the variants of an ensemble share their "
                    rf"structure\)$", text), text
    rc, msg, handle = _c_create(lib, [tabs[0], tabs[1], bad])
    assert rc == -1 and handle.value is None
    assert msg == text


def test_a_variant_with_another_wavelength_count_is_named(lib):
    tabs = E.tables("cooke")
    bad = copy.deepcopy(tabs[1])
    bad.optics = np.ascontiguousarray(bad.optics[:, :1])
    bad.wavelengths = bad.wavelengths[:1]
    with pytest.raises(StructureMismatch, match=r"variant 1: n_wl 1 differs from variant 0's 2"):
        check_structure([tabs[0], bad])
    short = copy.deepcopy(tabs[1])
    short.surfaces = short.surfaces[:-1].copy()
    with pytest.raises(StructureMismatch, match=r"variant 1: 7 surfaces differ from variant 0's 8"):
        check_structure([tabs[0], short])
    coeffs = copy.deepcopy(E.tables("singlet")[1])
    coeffs.coeffs = np.append(coeffs.coeffs, 0.0)
    with pytest.raises(StructureMismatch, match=r"variant 1: coefficient buffer of 4 values "
                                                r"differs from variant 0's 3") as exc:
        check_structure([E.tables("singlet")[0], coeffs])
    rc, msg, _h = _c_create(lib, [E.tables("singlet")[0], coeffs])
    assert rc == -1 and msg == str(exc.value)


def test_variants_that_differ_in_values_only_are_accepted(lib):
    """The fixture's variants: radii, thicknesses, indices, coefficients, and a tilt -- which sets
    SURF_ROTATED on one variant only: a statement about rot[], not structure."""
    for lens in E.LENSES:
        tabs = E.tables(lens)
        check_structure(tabs)
        flags = np.array([t.surfaces["flags"] for t in tabs])
        assert (flags & S.SURF_ROTATED).any() and not (flags[0] & S.SURF_ROTATED).any()
        rc, msg, _h = _c_create(lib, tabs)      # past every structure rule: it asks for a device
        assert (rc, msg) == (-3, "ol_ensemble_create: no HIP device (hipGetDevice failed)") \
            or rc == 0
    assert set(STRUCTURE_FIELDS) >= set(SURFACE_OF)


def test_what_no_ensemble_launch_serves_is_refused(lib):
    tabs = E.tables("cooke")
    forbes = copy.deepcopy(tabs[0])
    forbes.surfaces["geom_kind"][2] = S.GEOM_FORBES_Q
    forbes.surfaces["norm_radius"][2] = 10.0
    with pytest.raises(UnsupportedStructure, match="surface 2 is a Forbes surface"):
        check_structure([forbes])
    rc, msg, _h = _c_create(lib, [forbes])
    assert rc == -2 and "surface 2 is a Forbes surface" in msg
    newton = E.tables("singlet")[0]
    newton.surfaces["flags"][1] |= S.SURF_REFERENCE_NEWTON
    with pytest.raises(UnsupportedStructure, match="OL_SURF_REFERENCE_NEWTON"):
        check_structure([newton])
    rc, msg, _h = _c_create(lib, [newton])
    assert rc == -2 and "OL_SURF_REFERENCE_NEWTON" in msg


def test_entry_points_refuse_before_they_touch_a_device(lib):
    assert _capi.has_ensemble(lib)
    for name in ("ol_ensemble_create", "ol_ensemble_update", "ol_ensemble_destroy",
                 "ol_ensemble_size", "ol_trace_spot_ensemble"):
        assert name in _capi.EXPORTS
    assert lib.ol_ensemble_size(None) == 0
    lib.ol_ensemble_destroy(None)
    assert lib.ol_trace_spot_ensemble(None, 0, 4, None, 1, None, None, 0, None, None, None) == -1
    assert b"ensemble is NULL" in lib.ol_last_error()
    assert lib.ol_ensemble_update(None, 0, 1, None, None) == -1
    handle = C.c_void_p()
    assert lib.ol_ensemble_create(None, 0, 1, 1, C.byref(handle)) == -1
    assert b"no variants" in lib.ol_last_error()
    assert C.sizeof(_capi.EnsembleCell) == CELL_DTYPE.itemsize == 56


# ------------------------------------------------------------------ cells and moments
def test_cells_are_ordered_variant_field_wavelength():
    fields, wls = [(0.0, 0.0), (0.0, 0.7), (0.5, -0.5)], [2, 0]
    centers = np.arange(6, dtype=np.float64).reshape(3, 2)
    cells = cell_grid(4, fields, wls, centers=centers, vig=[(1, 1), (0.9, 0.8), (1, 1)])
    assert cells.shape == (4, 3, 2)
    flat = cells.reshape(-1)
    for k in range(4):
        for f in range(3):
            for w in range(2):
                c = flat[(k * 3 + f) * 2 + w]
                assert (c["variant"], c["wavelength_index"]) == (k, wls[w])
                assert (c["hx"], c["hy"]) == fields[f]
                assert (c["cx"], c["cy"]) == tuple(centers[f])
    assert flat[2]["vx"] == 0.9 and flat[2]["vy"] == 0.8 and flat[0]["vx"] == 1.0
    per_cell = np.zeros((4, 3, 2, 2))
    per_cell[3, 2, 1] = (7.0, 8.0)
    assert cell_grid(4, fields, wls, centers=per_cell)[3, 2, 1]["cy"] == 8.0
    with pytest.raises(ValueError, match="centers"):
        cell_grid(4, fields, wls, centers=np.zeros((2, 2)))


def test_radii_from_moments_are_spot_diagrams():
    """Hand-made hits -> the seven sums as the kernel forms them -> the (K, F, W) arithmetic,
    against `analysis.SpotDiagram`'s own methods on the same sums."""
    rng = np.random.default_rng(5)
    K, F, W, n = 2, 3, 2, 40
    centers = rng.normal(size=(F, 2))
    x = centers[None, :, None, 0, None] + 0.01 * rng.normal(size=(K, F, W, n))
    y = centers[None, :, None, 1, None] + 0.01 * rng.normal(size=(K, F, W, n))
    i = (rng.random((K, F, W, n)) > 0.1).astype(np.float64)
    dx, dy = x - centers[None, :, None, 0, None], y - centers[None, :, None, 1, None]
    lit = i > 0
    mom = np.zeros((K, F, W, 8))
    mom[..., 0] = lit.sum(-1)
    mom[..., 1], mom[..., 2] = (dx * lit).sum(-1), (dy * lit).sum(-1)
    mom[..., 3], mom[..., 4] = (dx * dx * lit).sum(-1), (dy * dy * lit).sum(-1)
    mom[..., 5] = i.sum(-1)
    mom[..., 6] = ((dx * dx + dy * dy) * lit).max(-1)
    cdx, cdy, rms, geo = radii_from_moments(mom)
    for k in range(K):
        sd = analysis.SpotDiagram.__new__(analysis.SpotDiagram)
        sd._moments = [[mom[k, f, w, :7] for w in range(W)] for f in range(F)]
        sd._centers = [tuple(c) for c in centers]
        sd._origin = np.zeros(3)
        for ref in range(W):
            sd.ref_index = ref
            want = np.array(sd.centroid())
            assert np.array_equal(centers[:, 0] + cdx[k, :, ref], want[:, 0])
            assert np.array_equal(centers[:, 1] + cdy[k, :, ref], want[:, 1])
        assert np.array_equal(rms[k], np.array(sd.rms_spot_radius()))
        assert np.array_equal(geo[k], np.array(sd.geometric_spot_radius()))
    # about the centroid: the operand's definition on the surviving rays
    want = np.array([[[E.operand_from_hits(x[k, f, w][lit[k, f, w]], y[k, f, w][lit[k, f, w]])
                       for w in range(W)] for f in range(F)] for k in range(K)])
    assert np.allclose(rms_about_centroid(mom), want, rtol=1e-9, atol=0)
    empty = np.zeros((1, 8))
    assert np.isnan(radii_from_moments(empty)[2][0]) and radii_from_moments(empty)[3][0] == 0.0


# ------------------------------------------------------------------ the host walk
def _case(tmp_path, lens, fp64, tables=None, cells=None):
    tabs, a = tables or E.tables(lens), E.arrays(lens)
    if cells is None:
        cells = cell_grid(len(tabs), a["fields"], E.wavelength_indices(lens, tabs[0]))
    path = os.path.join(str(tmp_path), f"{lens}_{int(fp64)}.bin")
    E.write_case(path, tabs, a["px"], a["py"], cells, fp64)
    return path, a, cells


@host
@pytest.mark.parametrize("fp64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("lens", E.LENSES)
def test_host_walk_is_each_variant_alone_and_holds_the_fixture(tmp_path, lens, fp64):
    path, a, cells = _case(tmp_path, lens, fp64)
    walk, rc, err = E.run_host("walk", path)
    assert rc == 0 and not err, err
    alone, rc, err = E.run_host("alone", path)
    assert rc == 0 and not err, err
    assert len(walk) == cells.size * E.N_RAYS + 1
    assert walk == alone                      # %.17g of every hit: bit for bit
    hits, status = E.parse_rays(walk, cells.size, E.N_RAYS)
    assert status == 0
    hits, want = hits.reshape(a["hits"].shape), a["hits"]
    tol = E.contract(lens, 64 if fp64 else 32)
    scale = float(np.abs(want[:, :, :, :2]).max())
    assert np.array_equal(hits[:, :, :, 2] > 0, want[:, :, :, 2] > 0)
    assert np.abs(hits[:, :, :, :2] - want[:, :, :, :2]).max() <= tol * scale
    assert np.abs(hits[:, :, :, 2] - want[:, :, :, 2]).max() <= tol
    if lens == "cooke":
        kept = (hits[:, :, :, 2] > 0).sum(-1)
        assert (kept[E.CLIPPED_VARIANT] < E.N_RAYS).any() and (kept[0] == E.N_RAYS).all()
    got = np.array([[[E.operand_from_hits(*hits[k, f, w, :2]) for w in range(hits.shape[2])]
                     for f in range(hits.shape[1])] for k in range(hits.shape[0])])
    assert np.abs(got - a["operand"]).max() <= tol * scale


@host
def test_host_walk_under_the_sanitizers(tmp_path):
    """The stand-alone program with AddressSanitizer + UndefinedBehaviorSanitizer linked in: the
    stacked tables, the variant strides and the cell walk read nothing they do not own -- also for
    cells that name a variant or a wavelength row outside the ensemble, which are skipped."""
    tabs = E.tables("singlet")
    cells = cell_grid(len(tabs), E.arrays("singlet")["fields"], [0, 1]).reshape(-1).copy()
    cells["variant"][3] = len(tabs)
    cells["variant"][4] = -1
    cells["wavelength_index"][5] = 2
    path, _a, _c = _case(tmp_path, "singlet", True, tabs, cells)
    plain, rc, err = E.run_host("walk", path)
    assert rc == 0 and not err, err
    checked, rc, err = E.run_host("walk", path, sanitize=True)
    assert rc == 0 and not err, err
    assert checked == plain
    hits, status = E.parse_rays(plain, cells.size, E.N_RAYS)
    assert status == _capi.STATUS_ENSEMBLE_CELL
    assert np.isnan(hits[3:6]).all() and not np.isnan(hits[:3]).any()


@host
def test_host_check_speaks_the_python_texts(tmp_path):
    tabs = E.tables("cooke")
    bad = _break(tabs[1], "aperture_kind")
    path, _a, _c = _case(tmp_path, "cooke", True, [tabs[0], bad])
    lines, rc, _err = E.run_host("check", path)
    with pytest.raises(StructureMismatch) as exc:
        check_structure([tabs[0], bad])
    assert rc == 0 and lines == [f"check: -1 {exc.value}"]


@host
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_host_walk_against_the_exact_trace(tmp_path, tag):
    """Three Cooke variants x one field against `_exact_front.gen_ray` +
    `_exact_trace.trace_ray` at 50 digits, under `_exact_trace.bound` (tests/_ensemble.py:
    exact_case) -- the host leg of tests/test_gpu_ensemble.py's check."""
    px, py, hx, hy = E.exact_inputs()
    cells = np.concatenate([cell_grid(6, [(hx, hy)], [E.EXACT_WL]).reshape(-1)[[k]]
                            for k in E.EXACT_VARIANTS])
    path = os.path.join(str(tmp_path), "exact.bin")
    E.write_case(path, E.tables("cooke"), px, py, cells, tag == "f64")
    lines, rc, err = E.run_host("walk", path)
    assert rc == 0 and not err, err
    hits, status = E.parse_rays(lines, cells.size, px.size)
    checks = E.exact_checks({k: hits[i] for i, k in enumerate(E.EXACT_VARIANTS)}, tag)
    for label, e, b in checks:
        print(f"[exact ensemble] host {tag} {label:60s} {e:.3e} / {b:.3e}")
    assert status == 0 and not [(lab, e, b) for lab, e, b in checks if not e <= b]


# ------------------------------------------------------------------ packing
@pytest.mark.reference
@pytest.mark.skipif(_live.reference_root() is None, reason="needs the reference package")
def test_pack_ensemble_restores_the_optic():
    _live.import_reference()
    from optiland_amd.packer import pack_ensemble, pack_optic
    optic = E.build_lens("cooke")
    wls = list(E.WAVELENGTHS["cooke"])
    before = pack_optic(optic, wls)
    radii = [22.0, 22.1, 22.2]

    def mutate(o, k):
        o.updater.set_radius(radii[k], 1)

    tabs = pack_ensemble(optic, mutate, 3, wls)
    assert [float(t.surfaces["radius"][1]) for t in tabs] == radii
    assert len({t.raygen["EPL"] for t in tabs}) == 3           # the entrance pupil moved
    check_structure(tabs)
    after = pack_optic(optic, wls)
    assert after.surfaces.tobytes() == before.surfaces.tobytes() and after.raygen == before.raygen
    # ... and with a restore callback the variants are made on the optic itself
    seen = []
    tabs2 = pack_ensemble(optic, mutate, 3, wls, restore=lambda o: (seen.append(1),
                                                                    o.updater.set_radius(22.01359, 1)))
    assert seen == [1] and [t.surfaces.tobytes() for t in tabs2] == \
        [t.surfaces.tobytes() for t in tabs]
    assert pack_optic(optic, wls).surfaces.tobytes() == before.surfaces.tobytes()
    # every table equals a fresh full pack of the mutated optic (the cached rows are current)
    fresh = E.build_lens("cooke")
    fresh.updater.set_radius(radii[2], 1)
    full = pack_optic(fresh, wls)
    assert full.surfaces.tobytes() == tabs[2].surfaces.tobytes()
    assert full.optics.tobytes() == tabs[2].optics.tobytes() and full.raygen == tabs[2].raygen


@pytest.mark.reference
@pytest.mark.skipif(_live.reference_root() is None, reason="needs the reference package")
def test_what_the_bridge_does_not_serve_is_refused_before_anything_moves():
    from optiland_amd.packer import UnsupportedSystem, pack_optic
    from optiland_amd.tolerancing import monte_carlo_spots
    problem = E.tolerancing_problem
    wls = [0.48, 0.55]
    tol = problem()
    before = pack_optic(tol.optic, wls)
    tol.add_compensator("thickness", surface_number=6)
    with pytest.raises(UnsupportedSystem, match="compensators"):
        monte_carlo_spots(tol, 4, "cpu")
    tol = problem()
    tol.add_operand("f2", dict(optic=tol.optic))
    with pytest.raises(UnsupportedSystem, match="operand 3 is 'f2'"):
        monte_carlo_spots(tol, 4, "cpu")
    tol = problem()
    tol.add_operand("rms_spot_size", dict(optic=tol.optic, surface_number=-1, Hx=0.0, Hy=0.0,
                                          num_rays=5, wavelength="all", distribution="hexapolar"))
    with pytest.raises(UnsupportedSystem, match="wavelength='all'"):
        monte_carlo_spots(tol, 4, "cpu")
    assert all(p.value is None for p in tol.perturbations)          # nothing was drawn
    after = pack_optic(tol.optic, wls)
    assert after.surfaces.tobytes() == before.surfaces.tobytes()
    # a perturbation that changes a surface's KIND is only known once it is applied: refused after
    # the replay, before anything is launched (no device is asked for), the optic nominal again
    from optiland import physical_apertures

    class ApertureOnEverySecondDraw:
        variable, value, calls = "aperture of surface 3", 0.0, 0

        def __init__(self, optic):
            self.optic = optic

        def apply(self):
            self.calls += 1
            self.value = float(self.calls % 2 == 0)
            self.optic.surfaces[3].aperture = \
                physical_apertures.RadialAperture(r_max=9.0) if self.value else None

        def reset(self):
            self.optic.surfaces[3].aperture = None

    tol = problem()
    tol.perturbations.append(ApertureOnEverySecondDraw(tol.optic))
    with pytest.raises(UnsupportedSystem, match="variant 1, surface 3: aperture_kind 1 differs"):
        monte_carlo_spots(tol, 4, "cpu")
    after = pack_optic(tol.optic, wls).surfaces     # (a thickness set and set back: to rounding)
    assert all(np.allclose(after[f], before.surfaces[f], rtol=1e-12, atol=1e-12, equal_nan=True)
               for f in after.dtype.names)
    # an optic that fails strict packing: refused before anything is drawn
    tol = problem()
    tol.optic.surfaces[3].interaction_model = object()
    with pytest.raises(UnsupportedSystem):
        pack_optic(tol.optic, wls)
    with pytest.raises(UnsupportedSystem):
        monte_carlo_spots(tol, 4, "cpu")
    assert all(p.value is None for p in tol.perturbations)
