"""Grid-sag surfaces without a GPU: the host build of optiland_amd/csrc/grid_sag_device.h
(tests/hostgrid) against the fixture tests/golden/grid_sag.npz and the reference's own known
answers, the cell choice against numpy.searchsorted, the sanitized stand-alone program on hostile
rays, the rules of ol_trace_grid_sag and of ol_system_create, the refusal of every range-walking
entry point, the packer, the change detector and the seam's switch.  Bounds and fixture:
tests/_grid_sag.py.
"""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from optiland_amd import system as S
from tests import _grid_sag as G
from tests import _live

REF = _live.reference_root() or _live.STAGED
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "optiland")),
                                     reason="reference package not present")
ROW = G.GRID


@pytest.fixture(scope="module")
def hostgrid():
    b = G._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return b.build()


# ------------------------------------------------------------------ the fixture itself
def test_fixture_holds_the_cases_and_keeps_its_margins():
    """Every case of the issue is there at both tolerances; at the reference's hit
    |sag(x, y) - z| <= 1e-13 for every ray that is not NaN (recomputed here in NumPy); a ray is NaN
    in position and direction or not at all; NaN rays in the narrow case only; every hit exactly on
    a grid line or LINE_MARGIN away; the nodes case has rays on nodes and along borders; uniform
    and non-uniform coordinates, a 2 x 2 grid, a tilted, a reflecting and a coated row occur."""
    assert G.case_names() == list(G.CASES)
    seen = set()
    for name in G.case_names():
        for tol in G.TOLS:
            c = G.case(name, tol)
            table, after = c["table"], c["after"]
            assert table.grid_sag_rows == (ROW,)
            assert float(table.surfaces["tol"][ROW]) == G.TOLS[tol]
            assert int(table.surfaces["max_iter"][ROW]) == 100
            n = {"hex469": 469, "hex127": 127, "nodes": 75}[G.CASES[name][2]]
            assert c["before"].shape == after.shape == c["lens"].shape == (8, n)
            assert not np.isnan(c["before"]).any()
            lost = np.isnan(after[0])
            assert np.array_equal(np.isnan(after[:6]).all(axis=0), lost)
            assert np.array_equal(np.isnan(after[:6]).any(axis=0), lost)
            assert lost.any() == (name in G.NAN_CASES)
            r = G.residual(table, ROW, after)
            assert np.array_equal(np.isnan(r), lost) and np.nanmax(r) <= G.RESIDUAL
            assert np.nanmax(r) == pytest.approx(G.golden()[f"{name}/residual"][list(G.TOLS).index(tol)])
            d = G.grid_line_distance(table, ROW, after)[:, ~lost]
            assert ((d == 0.0) | (d >= G.LINE_MARGIN)).all(), (name, float(d[d > 0].min()))
            if name == "nodes":
                assert ((d == 0).all(axis=0)).sum() >= 40 and ((d == 0).sum(axis=0) == 1).sum() >= 20
            if name == "clipped":
                assert 0 < (after[6] == 0).sum() < n
        xs, ys, z = G.block_of(table)
        seen.add((xs.size, ys.size))
        if np.ptp(np.diff(xs)) > 1e-9:
            seen.add("nonuniform")
        row = table.surfaces[ROW]
        seen.update(k for k, on in (("rotated", int(row["flags"]) & S.SURF_ROTATED),
                                    ("mirror", int(row["interaction"]) == S.INTERACT_REFLECT),
                                    ("coated", int(row["coating_kind"]) == S.COAT_SIMPLE),
                                    ("aperture", int(row["aperture_kind"]) != S.AP_NONE)) if on)
    assert {(33, 29), (5, 7), (2, 2), "nonuniform", "rotated", "mirror", "coated",
            "aperture"} <= seen


# ------------------------------------------------------------------ the host run of the device source
def _host_case(exe, tmp_path, c, dtype, tight, report=print):
    path = tmp_path / "step.case"
    G.write_case(path, c["table"], c["before"], c["g"], fp64=dtype is np.float64)
    got, bits = G.host_step(exe, path)
    what = f"{c['name']} tol {c['tol']:g}"
    G.compare(got, c["after"], dtype, G.scale_of(c["after"]), what, tight=tight, report=report)
    assert bool(bits & S.STATUS_NAN_DIRECTION) == bool(np.isnan(c["after"][3]).any()), what
    return got


@pytest.mark.parametrize("name", list(G.CASES))
def test_host_step_against_every_case(hostgrid, tmp_path, name):
    """fp64 within 1e-12 at tol = 1e-12; fp64 within 1e-6 and fp32 within 1e-4 at the factory
    tolerance; the same rays NaN as in the reference; the status bit exactly when there are."""
    _host_case(hostgrid, tmp_path, G.case(name, "tight"), np.float64, True)
    _host_case(hostgrid, tmp_path, G.case(name, "factory"), np.float64, False)
    _host_case(hostgrid, tmp_path, G.case(name, "factory"), np.float32, False)
    _host_case(hostgrid, tmp_path, G.case(name, "tight"), np.float32, False)


def test_host_step_gives_the_references_known_answers(hostgrid, tmp_path):
    """tests/test_grid_sag_geometry.py of the reference: the ray at (0, 0, -1) along +z onto the
    plane sag = 0.1 x travels 1.0 and is refracted at the normal (-0.1, 0, 1) / |.|."""
    gd = G.golden()
    table = S.SystemTable.from_json(str(gd["known_table"]))
    path = tmp_path / "known.case"
    G.write_case(path, table, gd["known_in"][:, None])
    got, bits = G.host_step(hostgrid, path)
    got = got[:, 0]
    z0 = float(table.surfaces["origin"][ROW][2])
    np.testing.assert_allclose(got[:3], [0.0, 0.0, z0], rtol=0, atol=1e-5)
    assert abs(got[7] - 1.0) <= 1e-5 and bits == 0
    np.testing.assert_allclose(got[3:6], gd["known_direction"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(got, gd["known_out"], rtol=0, atol=1e-12 * 10)


def _probe_coordinates(v: np.ndarray) -> np.ndarray:
    """Every node, nextafter either side of every node, both ends and beyond, cell centres."""
    out = [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf), 0.5 * (v[:-1] + v[1:]),
           [v[0] - 1.0, v[-1] + 1.0, v[0] - 1e30, v[-1] + 1e30, -np.inf, np.inf, 0.0]]
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in out])


@pytest.mark.parametrize("fp64", [True, False])
def test_cell_choice_is_searchsorted_right_minus_one_with_the_clamps(hostgrid, tmp_path, fp64):
    """grid_sag_cell against numpy.searchsorted(side="right") - 1 with the two clamps, on the
    coordinates as the table holds them (rounded to float in fp32): every node, nextafter either
    side of every node, both ends, far outside, +-inf; uniform, non-uniform, 2-node and 3-node
    vectors, x and y of different lengths; whatever cell the search starts from."""
    dt = np.float64 if fp64 else np.float32
    grids = [(G.axis(8.0, 33), G.axis(8.0, 29)), (G.axis(8.0, 33, 1.3), G.axis(6.0, 29, 1.3)),
             (np.array([-1.0, 1.0]), np.array([-1.0, 0.25, 1.0])),
             (np.cumsum(np.r_[0.0, np.logspace(-3, 1, 40)]) - 7.0, G.axis(3.0, 5, 2.0)),
             (G.axis(100.0, 512), G.axis(100.0, 257, 1.7))]
    for xs, ys in grids:
        table = G.table_with_grid(xs, ys, np.zeros((ys.size, xs.size)))
        xs_t, ys_t = xs.astype(dt), ys.astype(dt)
        probe = np.concatenate([_probe_coordinates(xs_t.astype(np.float64)),
                                _probe_coordinates(ys_t.astype(np.float64))])
        if not fp64:   # nextafter in the table's own precision
            probe = np.concatenate([probe, np.nextafter(xs_t, dt(-np.inf)), np.nextafter(xs_t, dt(np.inf)),
                                    np.nextafter(ys_t, dt(-np.inf)), np.nextafter(ys_t, dt(np.inf))]
                                   ).astype(np.float64)
        path = tmp_path / "cells.case"
        G.write_case(path, table, np.zeros((8, 1)), 1, fp64=fp64, probe=probe)
        ix, iy = G.host_cells(hostgrid, path)
        p = probe.astype(dt)
        np.testing.assert_array_equal(ix, G.cell_numpy(xs_t, p))
        np.testing.assert_array_equal(iy, G.cell_numpy(ys_t, p))
        assert ix.min() == 0 and ix.max() == xs.size - 2 and iy.max() == ys.size - 2


def _hostile_rays(c):
    """The case's first rays with NaN, +-inf and 1e30 put into every position and direction plane
    in turn, and rays that are hostile everywhere; and which of them cannot have a hit (NaN or inf
    somewhere: a ray from z = -1e30 along +z does reach the surface)."""
    base = c["before"][:, :4]
    out, lost = [base], [np.zeros(4, dtype=bool)]
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for plane in range(6):
            r = base.copy()
            r[plane] = bad
            out.append(r)
            lost.append(np.full(4, not np.isfinite(bad)))
        r = base.copy()
        r[:6] = bad
        out.append(r)
        lost.append(np.full(4, not np.isfinite(bad)))
    return np.concatenate(out, axis=1), np.concatenate(lost)


def test_host_step_under_the_sanitizers(tmp_path):
    """The same program built with AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone
    program: the runtime is linked into it) runs the fixture bundles clean, then rays with NaN,
    +-inf and 1e30 positions and directions on a table whose coefficient buffer IS the grid block
    -- any load outside the block is a heap overflow the sanitizer reports -- and its other
    modes.  Host only: the out-of-range-read check."""
    b = G._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    if not G.sanitizers_available(tmp_path):
        pytest.skip("this box cannot build or run a sanitized program at all")
    exe = b.build(sanitize=True)     # (a failure to build the checker is a failure)
    for name in G.CASES:
        _host_case(exe, tmp_path, G.case(name, "tight"), np.float64, True, report=None)
        _host_case(exe, tmp_path, G.case(name, "factory"), np.float32, False, report=None)
    path = tmp_path / "hostile.case"
    for name in ("uniform", "nonuniform", "plane2x2", "tilted"):
        c = G.case(name, "factory")
        rays, lost = _hostile_rays(c)
        for fp64 in (True, False):
            G.write_case(path, c["table"], rays, fp64=fp64)
            got, _bits = G.host_step(exe, path)
            assert got.shape == rays.shape
            # the untouched rays come out with a hit, a ray with a NaN or an inf without one
            assert not np.isnan(got[:, :4]).any()
            assert np.isnan(got[:3, lost]).any(axis=0).all()
    xs, ys = G.axis(8.0, 33, 1.3), G.axis(8.0, 29)
    alone = G.table_with_grid(xs, ys, G.sag_table(xs, ys, 30.0))
    rays = np.zeros((8, 4))
    rays[0], rays[1], rays[2], rays[5], rays[6] = [0.0, 1.3, -7.9, 7.99], 0.4, -2.0, 1.0, 1.0
    hostile, lost = _hostile_rays({"before": rays})
    for fp64 in (True, False):
        G.write_case(path, alone, hostile, 1, fp64=fp64, probe=_probe_coordinates(xs))
        got, _bits = G.host_step(exe, path)
        assert not np.isnan(got[:, :4]).any() and np.isnan(got[:3, lost]).any(axis=0).all()
        G.host_cells(exe, path)
    G.write_case(path, G.case("uniform")["table"], G.case("uniform")["before"])
    assert "ol_trace: -2" in G.run_host(exe, "refuse", path)
    assert "good: 0 ok" in G.run_host(exe, "rules", path)
    assert "create: 0 ok" in G.run_host(exe, "create", path)


# ------------------------------------------------------------------ rules and refusals
def _lines(text):
    out = {}
    for line in text.splitlines():
        what, rest = line.split(": ", 1)
        code, _, msg = rest.partition(" ")
        out[what] = (int(code), msg)
    return out


def test_every_range_walking_entry_refuses_a_grid_sag_row(hostgrid, tmp_path):
    """OL_EUNSUPPORTED naming the surface, before any launch."""
    for name in ("uniform", "plane2x2", "mirror"):
        c = G.case(name)
        path = tmp_path / "refuse.case"
        G.write_case(path, c["table"], c["before"][:, :1])
        got = _lines(G.run_host(hostgrid, "refuse", path))
        for who in ("ol_trace", "ol_trace one surface", "ol_trace_ex", "ol_newton_count",
                    "ol_trace_generate", "ol_trace_spot", "ol_trace_spot_batch", "ol_trace_opd",
                    "ol_wavefront_reference", "ol_trace_opd_dev", "ol_aim_rays"):
            assert got[who][0] == -2 and "surface 2 is a grid-sag surface" in got[who][1], \
                (who, got[who])
        assert got["ol_trace"][1] == ("ol_trace: surface 2 is a grid-sag surface: trace it with "
                                      "ol_trace_grid_sag and cut the range there")


def test_argument_rules_on_a_host_system(hostgrid, tmp_path):
    """ol_trace_grid_sag's host rules (csrc/grid_sag_host.h) without a device: the rules and the
    texts of ol_trace_forbes."""
    c = G.case("clipped")
    path = tmp_path / "rules.case"
    G.write_case(path, c["table"], c["before"])
    got = _lines(G.run_host(hostgrid, "rules", path))
    for ok in ("good", "good fp32 midrange", "empty"):
        assert got[ok] == (0, "ok"), ok
    who = "ol_trace_grid_sag: "
    for what, code, text in (
            ("null system", -1, "system is NULL"), ("dtype", -1, "bad dtype 5"),
            ("negative count", -1, "negative ray count"),
            ("surface -1", -1, "surface -1 outside [0, 5)"),
            ("surface past the table", -1, "surface 5 outside [0, 5)"),
            ("not a grid-sag row", -1, "surface 3 is not a grid-sag surface (geometry kind 1): "
                                       "trace it with ol_trace"),
            ("wavelength", -1, "wavelength index 1 outside [0, 1)"),
            ("wavelength -1", -1, "wavelength index -1 outside [0, 1)"),
            ("flags", -1, "flags 0x4: OL_TRACE_WRITE_RAYS and OL_TRACE_MIDRANGE only"),
            ("too many", -1, "137438953409 rays are more than one launch takes"),
            ("null rays", -1, "rays is NULL"), ("null plane", -1, "rays[5] is NULL"),
            ("stride", -1, "record_stride 126 < n_rays 127"),
            ("nothing to write", -1, "nothing to write (no record_row, no OL_TRACE_WRITE_RAYS)")):
        assert got[what] == (code, who + text), (what, got[what])
    coated = S.SystemTable.from_json(c["table"].to_json())
    coated.surfaces["coating_kind"][ROW] = S.COAT_FRESNEL
    G.write_case(path, coated, c["before"])
    got = _lines(G.run_host(hostgrid, "rules", path))
    assert got["good"] == (-2, who + "surface 2 carries a polarisation-dependent coating "
                                     "(unpolarised launches only)")


def test_system_create_validates_grid_sag_blocks(hostgrid, tmp_path):
    """Every rule of the block, each answered with a text that names the surface and the rule;
    kinds 13, 15 and 17 stay refused with the text they always had."""
    def create(table):
        path = tmp_path / "create.case"
        G.write_case(path, table, np.zeros((8, 1)), 1)
        return _lines(G.run_host(hostgrid, "create", path))["create"]

    xs, ys = G.axis(4.0, 5), G.axis(3.0, 4, 1.3)
    z = G.sag_table(xs, ys, 30.0)
    W, H = xs.size, ys.size

    def table(block=None, n_coeff=None):
        t = G.table_with_grid(xs, ys, z)
        if block is not None:
            t.coeffs = np.asarray(block, dtype=np.float64)
            t.surfaces["n_coeff"][1] = t.coeffs.size if n_coeff is None else n_coeff
        return t

    def refused(t, *words, code=-1):
        got = create(t)
        assert got[0] == code and got[1].startswith("surface 1: ") \
            and all(w in got[1] for w in words), (words, got)

    good = table().coeffs.copy()
    assert create(table()) == (0, "ok")
    assert create(G.table_with_grid([-1.0, 1.0], [-1.0, 1.0], np.zeros((2, 2)))) == (0, "ok")

    def put(at, value):
        b = good.copy()
        b[at] = value
        return b

    for at in (0, 1):        # W, H >= 2 and whole
        for bad in (1.0, 0.0, -3.0, 2.5, np.nan, np.inf, 1e9):
            refused(table(put(at, bad)), "W, H >= 2")
    refused(table(good[:1]), "W, H >= 2")
    # counts add up to n_coeff exactly
    refused(table(good[:-1]), "does not match the counts")
    refused(table(np.append(good, 0.0)), "does not match the counts")
    refused(table(put(0, W + 1.0)), "does not match the counts")
    # every value finite
    for at in (2, 2 + W - 1, 2 + W, 2 + W + H - 1, 2 + W + H, good.size - 1):
        for bad in (np.nan, np.inf, -np.inf):
            refused(table(put(at, bad)), "not finite")
    # strictly increasing, as doubles and as floats
    refused(table(put(3, good[2])), "x coordinates", "strictly increasing")
    refused(table(put(3, good[4] + 1.0)), "x coordinates", "strictly increasing")
    refused(table(put(2 + W + 1, good[2 + W])), "y coordinates", "strictly increasing")
    refused(table(put(2 + W + 2, good[2 + W] - 1.0)), "y coordinates", "strictly increasing")
    near = float(np.nextafter(np.float32(good[2]), np.float32(np.inf)))
    assert good[2] < good[2] + 0.25 * (near - good[2]) and \
        np.float32(good[2] + 0.25 * (near - good[2])) == np.float32(good[2])
    refused(table(put(3, good[2] + 0.25 * (near - good[2]))), "x coordinates", "as floats")
    # a block that runs past the buffer, a row that only records
    t = table()
    t.surfaces["n_coeff"][1] += 1
    assert create(t)[0] == -1 and "exceeds the buffer" in create(t)[1]
    t = table()
    t.surfaces["interaction"][1] = S.INTERACT_RECORD_ONLY
    assert create(t) == (-2, "surface 1: a grid-sag surface that only records")
    for kind in (13, 15, 17):
        t = table()
        t.surfaces["geom_kind"][1] = kind
        assert create(t) == (-2, f"surface 1: geometry kind {kind}")


def test_python_layers_know_the_new_kind_and_the_library_exports_the_entry():
    from optiland_amd import _capi, build

    assert S.GEOM_GRID_SAG == 16 == _capi.GEOM_GRID_SAG
    assert S.GEOM_NAMES[16] == "grid_sag" and not {13, 15, 17} & set(S.GEOM_NAMES)
    assert "ol_trace_grid_sag" in _capi.EXPORTS and _capi.ABI_VERSION == 11
    header = open(os.path.join(_live.ROOT, "include", "optiland_hip.h")).read()
    assert "OL_GEOM_GRID_SAG = 16" in header and "int ol_trace_grid_sag(" in header
    assert "#define OL_ABI_VERSION 11" in header
    build.build_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.library_path()], text=True)
    assert " T ol_trace_grid_sag" in out
    lib = _capi.load()
    assert _capi.has_trace_grid_sag(lib) and lib.ol_abi_version() == 11
    rc = lib.ol_trace_grid_sag(None, _capi.F64, 1, None, 0, None, 0, 1, 1, None, None)
    assert rc == -1 and lib.ol_last_error() == b"ol_trace_grid_sag: system is NULL"
    t = G.case("uniform")["table"]
    again = S.SystemTable.from_json(t.to_json())
    assert again.grid_sag_rows == (ROW,) == t.grid_sag_rows
    assert again.forbes == () and again.gratings == () and again.phases == ()
    assert again.reference_newton_surfaces() == []


def test_engine_and_tracer_declare_the_capability():
    import optiland_amd.tracer as tr
    from optiland_amd.engine import HipSystem

    assert tr._make_engine.traces_grid_sags is True
    assert callable(HipSystem.can_trace_grid_sag) and callable(HipSystem.trace_grid_sag)


# ------------------------------------------------------------------ with the live reference
@pytest.fixture(scope="module")
def ref():
    shim = os.path.join(os.path.dirname(os.path.abspath(__file__)), "refshim")
    sys.dont_write_bytecode = True
    added = [p for p in (shim, REF) if p not in sys.path]
    sys.path[:0] = added
    import optiland.backend as be
    be.set_backend("numpy")
    yield be
    be.set_backend("numpy")
    for p in added:
        sys.path.remove(p)


@needs_reference
def test_packer_packs_the_documented_row_and_block(ref):
    """The reference's own optic -- surface type "grid_sag" through its factory -- goes to kind 16
    with the geometry's tol and max_iter and the block {W, H, x, y, sag row-major}; strict packing
    and a pack without `grid_sags` keep refusing it; the fixture's tables are what it packs."""
    from optiland_amd.packer import UnsupportedSystem, pack_optic, pack_surfaces

    lens = G.case_lens("nonuniform", 1e-9)
    geom = lens.surfaces.surfaces[ROW].geometry
    assert type(geom).__name__ == "GridSagGeometry"
    geom.max_iter = 37
    t = G.packed(lens)
    assert t.grid_sag_rows == (ROW,) and t.unsupported == ()
    row = t.surfaces[ROW]
    assert int(row["geom_kind"]) == S.GEOM_GRID_SAG == 16
    assert float(row["tol"]) == 1e-9 and int(row["max_iter"]) == 37
    assert np.isinf(float(row["radius"])) and not int(row["flags"]) & S.SURF_REFERENCE_NEWTON
    xs, ys, z = G.block_of(t)
    np.testing.assert_array_equal(xs, np.asarray(geom.x_grid))
    np.testing.assert_array_equal(ys, np.asarray(geom.y_grid))
    np.testing.assert_array_equal(z, np.asarray(geom.sag_grid))
    assert z.shape == (29, 33) and z[3, 5] == float(np.asarray(geom.sag_grid)[3, 5])
    with pytest.raises(UnsupportedSystem):
        pack_optic(lens)
    with pytest.raises(UnsupportedSystem):
        pack_surfaces(lens.surfaces.surfaces, [G.WAVELENGTH])
    loose = pack_surfaces(lens.surfaces.surfaces, [G.WAVELENGTH], tolerate=True)
    assert loose.grid_sag_rows == () and loose.unsupported == (ROW,)
    for name in G.CASES:
        want = G.case(name, "factory")["table"]
        got = G.packed(G.case_lens(name))
        assert got.to_json() == want.to_json(), name
    # on the torch backend the arrays are tensors: the same block
    ref.set_backend("torch")
    ref.set_device("cpu")
    ref.set_precision("float64")
    try:
        t2 = G.packed(G.case_lens("nonuniform", 1e-9))
        np.testing.assert_array_equal(t2.coeffs, G.packed(lens).coeffs)
    finally:
        ref.set_backend("numpy")


@needs_reference
def test_packer_leaves_these_to_the_reference(ref):
    """A subclass, values that are not finite, coordinates that are not strictly increasing (as
    doubles, as floats), a shape mismatch, fewer than 2 nodes on an axis, a BSDF, a Jones coating,
    an inhomogeneous medium, the opt-in reference Newton rule: each stays in `table.unsupported`."""
    from optiland.coatings import FresnelCoating
    from optiland.geometries.grid_sag import GridSagGeometry

    def left(lens):
        t = G.packed(lens)   # (a medium is shared with the next surface: that one may go too)
        return t.grid_sag_rows == () and ROW in t.unsupported

    def geom(lens):
        return lens.surfaces.surfaces[ROW].geometry

    assert not left(G.lens())

    class Mine(GridSagGeometry):
        pass

    lens = G.lens()
    geom(lens).__class__ = Mine
    assert left(lens)
    for bad in (np.nan, np.inf):
        lens = G.lens()
        geom(lens).sag_grid[3, 4] = bad
        assert left(lens)
        lens = G.lens()
        geom(lens).y_grid[-1] = bad
        assert left(lens)
    lens = G.lens()
    geom(lens).tol = float("nan")
    assert left(lens)
    lens = G.lens()
    geom(lens).x_grid[4] = geom(lens).x_grid[3]                 # equal
    assert left(lens)
    lens = G.lens()
    geom(lens).x_grid = geom(lens).x_grid[::-1].copy()          # decreasing
    assert left(lens)
    lens = G.lens()
    geom(lens).y_grid[4] = geom(lens).y_grid[3] + 1e-12         # increasing, not as floats
    assert geom(lens).y_grid[4] > geom(lens).y_grid[3]
    assert left(lens)
    lens = G.lens()
    geom(lens).sag_grid = geom(lens).sag_grid[:, :-1].copy()    # shape mismatch
    assert left(lens)
    lens = G.lens()
    geom(lens).x_grid = geom(lens).x_grid[:1].copy()            # one node on an axis
    geom(lens).sag_grid = geom(lens).sag_grid[:, :1].copy()
    assert left(lens)
    lens = G.lens()
    lens.surfaces.surfaces[ROW].interaction_model.bsdf = object()
    assert left(lens)
    lens = G.lens()
    surf = lens.surfaces.surfaces[ROW]
    surf.interaction_model.coating = FresnelCoating(surf.material_pre, surf.material_post)
    assert left(lens)
    lens = G.lens()

    class Grin:
        pass

    Grin.__name__ = "GrinPropagation"
    surf = lens.surfaces.surfaces[ROW]
    was = surf.material_post.propagation_model
    surf.material_post.propagation_model = Grin()
    try:
        assert left(lens)
    finally:
        surf.material_post.propagation_model = was
    was = S.OPTIONS["reference_newton"]
    S.OPTIONS["reference_newton"] = True
    try:
        assert left(G.lens())
    finally:
        S.OPTIONS["reference_newton"] = was
    assert not left(G.lens())


@needs_reference
@pytest.mark.parametrize("native", [True, False])
def test_surface_token_changes_with_the_grid(ref, native):
    """x_grid, y_grid, sag_grid (in place and reassigned), tol, max_iter; and the reference's own
    GridSagVariable update between two traces."""
    from optiland.optimization.variable.grid_sag import GridSagVariable
    from optiland_amd import fingerprint as fp

    if native and fp._NATIVE is None:
        from optiland_amd import build

        build.build_fptoken(force=False, verbose=False)
        fp._NATIVE = fp._load_native()
        assert fp._NATIVE is not None, "csrc/fptoken.c built but does not load"
    assert fp.use_native(native) is native

    def token(lens):
        tok, _keep = fp.surfaces_token(lens.surfaces.surfaces, G.WAVELENGTH)
        return tok[1][ROW]

    def node(g):
        g.sag_grid[2, 3] += 1e-3

    def variable(lens):
        var = GridSagVariable(lens, ROW)
        var.update_value(var.get_value() * 1.01)

    edits = [("a node in place", node),
             ("an x coordinate in place", lambda g: g.x_grid.__setitem__(0, g.x_grid[0] - 0.01)),
             ("y reassigned", lambda g: setattr(g, "y_grid", g.y_grid * 1.01)),
             ("sag reassigned", lambda g: setattr(g, "sag_grid", g.sag_grid * 0.5)),
             ("tol", lambda g: setattr(g, "tol", 1e-9)),
             ("max_iter", lambda g: setattr(g, "max_iter", 50))]
    try:
        for backend in ("numpy", "torch"):
            ref.set_backend(backend)
            if backend == "torch":
                ref.set_device("cpu")
                ref.set_precision("float64")
            for what, edit in edits:
                lens = G.lens()
                before = token(lens)
                assert before == token(lens), what
                edit(lens.surfaces.surfaces[ROW].geometry)
                assert before != token(lens), (backend, what)
            lens = G.lens()
            before, packed = token(lens), G.packed(lens)
            variable(lens)
            assert before != token(lens), (backend, "GridSagVariable")
            again = G.packed(lens)
            np.testing.assert_allclose(G.block_of(again)[2], 1.01 * G.block_of(packed)[2],
                                       rtol=1e-15)
    finally:
        fp.use_native(fp._NATIVE is not None)
        ref.set_backend("numpy")


@needs_reference
def test_a_factory_that_declares_nothing_gets_todays_table(ref, monkeypatch):
    """The seam decides before packing: an engine factory without `traces_grid_sags` (every
    stand-in of the existing suite) never sees a grid-sag row, and neither does anyone after
    `enable(grid_sags=False)`."""
    import optiland_amd.tracer as tr
    from optiland_amd import integration as I

    monkeypatch.setitem(I._SG, "grid_sags", True)
    lens = G.lens()
    t = I._sg_table(lens.surfaces, G.WAVELENGTH)
    assert t.grid_sag_rows == (ROW,) and t.unsupported == ()
    monkeypatch.setitem(I._SG, "grid_sags", False)
    t = I._sg_table(lens.surfaces, G.WAVELENGTH)
    assert t.grid_sag_rows == () and t.unsupported == (ROW,)
    monkeypatch.setitem(I._SG, "grid_sags", True)
    monkeypatch.setattr(tr, "_make_engine", lambda table, device: None)
    t = I._sg_table(lens.surfaces, G.WAVELENGTH)
    assert t.grid_sag_rows == () and t.unsupported == (ROW,)


@needs_reference
def test_enable_takes_the_switch(ref):
    from optiland_amd import integration as I

    was = I._SG["grid_sags"]
    try:
        I.enable(force=True, analyses=False, grid_sags=False)
        assert I._SG["grid_sags"] is False
        I.enable(force=True, analyses=False)
        assert I._SG["grid_sags"] is False     # None leaves it as it is
        I.enable(force=True, analyses=False, grid_sags=True)
        assert I._SG["grid_sags"] is True
    finally:
        I.disable()
        I._SG["grid_sags"] = was


# ------------------------------------------------------------------ the drop-in, end to end on CPU
@pytest.fixture()
def grid_sag_on_cpu(ref, monkeypatch, hostgrid, tmp_path):
    import optiland_amd.tracer as tr
    from optiland_amd import integration as I

    cls = G.make_engine_class(hostgrid, tmp_path)
    cls.grid_sag_launches = 0

    def factory(table, device):
        return cls(table, device)

    factory.traces_grid_sags = True    # what the product's own factory declares
    monkeypatch.setattr(tr, "_make_engine", factory)
    monkeypatch.setitem(I._SG, "grid_sags", True)
    be = ref
    be.set_backend("torch")
    be.set_device("cpu")
    be.set_precision("float64")
    yield be, cls
    be.set_backend("numpy")


def _recorded(be, lens):
    return np.stack([np.stack([np.asarray(be.to_numpy(getattr(s, k)), dtype=np.float64).reshape(-1)
                               for k in ("x", "y", "z", "L", "M", "N", "intensity", "opd")])
                     for s in lens.surfaces.surfaces])


def _reference_rows(be, name, polarized=False):
    """What the reference's own `Optic.trace` records for the case's field: an optic of its own,
    nothing installed on it."""
    lens = G.case_lens(name, G.TOLS["tight"])
    if polarized:
        from optiland.rays import PolarizationState
        lens.updater.set_polarization(PolarizationState(is_polarized=False))
    hx, hy = G.CASES[name][1]
    lens.trace(hx, hy, G.WAVELENGTH, 6, "hexapolar")
    return _recorded(be, lens)


@needs_reference
@pytest.mark.parametrize("name", ["uniform", "nonuniform", "mirror", "narrow"])
def test_dropin_traces_the_grid_sag_surface_on_the_engine(grid_sag_on_cpu, name):
    """The bridged `SurfaceGroup.trace` with a grid-sag row: one launch of the engine's
    `trace_grid_sag`, no surface to the reference's own trace, every recorded row equal to the
    reference's own trace of the same bundle to the fp64 bound (the narrow case with its NaN
    rays)."""
    (be, cls) = grid_sag_on_cpu
    from optiland_amd import integration as I

    want = _reference_rows(be, name)
    lens = G.case_lens(name, G.TOLS["tight"])
    I.install(lens, force=True)
    foreign, served = I._SG["foreign"], I._SG["count"]
    hx, hy = G.CASES[name][1]
    lens.trace(hx, hy, G.WAVELENGTH, 6, "hexapolar")
    assert I._SG["count"] == served + 1          # the group's trace was the bridge's
    assert I._SG["foreign"] == foreign           # and no surface went to the reference's own trace
    assert cls.grid_sag_launches == 1
    got = _recorded(be, lens)
    assert got.shape == want.shape and got.shape[2] == 127
    assert bool(np.isnan(want[ROW, 0]).any()) == (name in G.NAN_CASES)
    G.compare(got, want, np.float64, G.scale_of(want), name, tight=True, report=print)


@needs_reference
def test_dropin_polarised_bundle_takes_the_references_surface(grid_sag_on_cpu):
    """A polarised bundle: no `trace_grid_sag` launch, the surface goes to the reference's own
    `Surface.trace` (one foreign surface), and the rows are the reference's own."""
    (be, cls) = grid_sag_on_cpu
    from optiland.rays import PolarizationState
    from optiland_amd import integration as I

    want = _reference_rows(be, "uniform", polarized=True)
    lens = G.case_lens("uniform", G.TOLS["tight"])
    lens.updater.set_polarization(PolarizationState(is_polarized=False))
    I.install(lens, force=True)
    foreign, served = I._SG["foreign"], I._SG["count"]
    lens.trace(0.0, 1.0, G.WAVELENGTH, 6, "hexapolar")
    assert cls.grid_sag_launches == 0
    assert I._SG["foreign"] == foreign + 1 and I._SG["count"] == served + 1
    got = _recorded(be, lens)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * G.scale_of(want))


@needs_reference
def test_dropin_switch_and_subclass_send_the_surface_back_to_the_reference(grid_sag_on_cpu):
    (be, cls) = grid_sag_on_cpu
    from optiland.geometries.grid_sag import GridSagGeometry
    from optiland_amd import integration as I

    want = _reference_rows(be, "uniform")
    I._SG["grid_sags"] = False   # what enable(grid_sags=False) / OPTILAND_HIP_GRID_SAGS=0 set
    lens = G.case_lens("uniform", G.TOLS["tight"])
    I.install(lens, force=True)
    foreign = I._SG["foreign"]
    lens.trace(0.0, 1.0, G.WAVELENGTH, 6, "hexapolar")
    assert cls.grid_sag_launches == 0 and I._SG["foreign"] == foreign + 1
    np.testing.assert_allclose(_recorded(be, lens), want, rtol=0, atol=1e-12 * G.scale_of(want))
    I._SG["grid_sags"] = True    # and back on: the same lens, the next trace
    lens.trace(0.0, 1.0, G.WAVELENGTH, 6, "hexapolar")
    assert cls.grid_sag_launches == 1 and I._SG["foreign"] == foreign + 1

    class Mine(GridSagGeometry):
        pass

    lens.surfaces.surfaces[ROW].geometry.__class__ = Mine
    lens.trace(0.0, 1.0, G.WAVELENGTH, 6, "hexapolar")
    assert cls.grid_sag_launches == 1 and I._SG["foreign"] == foreign + 2
    np.testing.assert_allclose(_recorded(be, lens), want, rtol=0, atol=1e-12 * G.scale_of(want))
