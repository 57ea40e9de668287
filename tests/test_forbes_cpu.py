"""Forbes surfaces without a GPU: the host build of optiland_amd/csrc/forbes_device.h
(tests/hostforbes) against the fixture tests/golden/forbes.npz, the table rules of
ol_system_create, the refusal of every range-walking entry point, the packer, the change
detector and the drop-in end to end on CPU tensors.  Bounds and fixture: tests/_forbes.py.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from optiland_amd import system as S
from tests import _forbes as F
from tests import _live

REF = _live.reference_root() or _live.STAGED
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "optiland")),
                                     reason="reference package not present")


@pytest.fixture(scope="module")
def hostforbes():
    b = F._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return b.build()


# ------------------------------------------------------------------ host build against the fixture
@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("variant", ["norm12", "flat"])
def test_host_sag_and_normal_on_the_grid(hostforbes, tmp_path, kind, variant):
    """sag and unit normal on the 33 x 33 grid over u <= 1.2 and the extra points: the vertex, u
    just inside and outside 1, infinite base radius and k != 0 (norm12: R 40, k -0.5)."""
    g = F.grid(kind, variant)
    x, y = g["x"], g["y"]
    norm = float(g["table"].surfaces[F.FORBES]["norm_radius"])
    u = np.hypot(x, y) / norm
    assert np.any((x == 0) & (y == 0)) and np.any((u < 1) & (u > 1 - 2e-9)) \
        and np.any((u > 1) & (u < 1 + 2e-9)) and u.max() > 1.2
    planes = np.zeros((8, x.size))
    planes[0], planes[1] = x, y
    path = tmp_path / "grid.case"
    F.write_case(path, g["table"], planes)
    got = F.host_grid(hostforbes, path)
    keep = np.ones(x.size, dtype=bool)
    if kind == "q2d":
        keep = np.abs(u - 1.0) >= F.EDGE
    assert not np.isnan(got).any() and not np.isnan(g["sag"]).any()
    e_sag = np.abs(got[0] - g["sag"])[keep].max()
    e_nrm = np.abs(got[1:] - g["normal"])[:, keep].max()
    print(f"grid {kind} {variant}: sag {e_sag:.3g} (bound {F.grid_bound(g, 'sag'):.3g}), "
          f"normal {e_nrm:.3g} (bound {F.grid_bound(g, 'normal'):.3g})")
    assert e_sag <= F.grid_bound(g, "sag")
    assert e_nrm <= F.grid_bound(g, "normal")
    # the departure is cut outside the disc: only the base conic is left there
    out = u > 1 + F.EDGE
    base = F.grid(kind, variant)["table"]
    row = base.surfaces[F.FORBES]
    r2 = (x * x + y * y)[out]
    R, k = float(row["radius"]), float(row["conic"])
    conic = np.zeros_like(r2) if np.isinf(R) else \
        r2 / (R * (1 + np.sqrt(np.maximum(1 - (1 + k) * r2 / R ** 2, 0.0))))
    assert np.abs(got[0][out] - conic).max() <= 1e-14


@pytest.mark.parametrize("name", F.case_names())
def test_host_step_against_every_case(hostforbes, tmp_path, name):
    """The one-surface step, ray set by ray set (N = 127, 1 and, in the norm8 cases, 1027), fp64
    and fp32: the Forbes surface's recorded row from the row in front of it."""
    c = F.case(name)
    assert set(c["sets"]) >= set(F.RAYSETS) and (F.BIG_SET in c["sets"]) == (c["variant"] == "norm8")
    assert c["edge"].mean() <= F.EDGE_CAP
    for dtype in (np.float64, np.float32):
        for rayset, (lo, hi) in c["sets"].items():
            assert hi - lo == {"hex127": 127, "chief": 1, F.BIG_SET: 1027}[rayset]
            path = tmp_path / "step.case"
            F.write_case(path, c["table"], c["rows"][F.FORBES - 1][:, lo:hi],
                         fp64=dtype is np.float64)
            got, bits = F.host_step(hostforbes, path)
            assert bits == 0
            F.compare(got[None], c, dtype, lo, hi, rows=[F.FORBES], report=print)


def test_host_step_under_the_sanitizers(tmp_path):
    """The same program built with AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone
    program: the runtime is linked into it): every read of the table, of the coefficient blocks
    and of the ray planes that the sweeps make is checked, Q and Q2D, fp64 and fp32, a ray count
    that is no multiple of anything, and the refusals."""
    b = F._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    try:
        exe = b.build(sanitize=True)
    except Exception as exc:  # noqa: BLE001 - no sanitizer runtime on this box
        pytest.skip(f"sanitized build not available: {exc}")
    for name in ("q_norm8_default", "q2d_norm8_default", "q2d_tilted_tight"):
        c = F.case(name)
        lo, hi = c["sets"]["hex127"]
        for fp64 in (True, False):
            path = tmp_path / "asan.case"
            F.write_case(path, c["table"], c["rows"][0][:, lo:hi], fp64=fp64)
            got, _bits = F.host_step(exe, path)
            F.compare(got[None], c, np.float64 if fp64 else np.float32, lo, hi, rows=[F.FORBES])
        assert "ol_trace: -2" in F.run_host(exe, "refuse", path)
        assert "good: 0 ok" in F.run_host(exe, "rules", path)
        g = F.grid(c["kind"], "norm12")
        planes = np.zeros((8, g["x"].size))
        planes[0], planes[1] = g["x"], g["y"]
        F.write_case(path, g["table"], planes)
        assert F.host_grid(exe, path).shape == (4, g["x"].size)


def test_host_status_and_nan_pattern(hostforbes, tmp_path):
    """A ray that misses the base conic is NaN, a totally reflected one keeps its position and
    raises the informational bit; their neighbours are untouched."""
    c = F.case("q_norm12_tight")
    rays = np.repeat(c["rows"][0][:, :1], 3, axis=1)
    rays[1, 1] = 500.0                      # far outside R = 40: no intersection with the conic
    flipped = S.SystemTable.from_json(c["table"].to_json())
    path = tmp_path / "nan.case"
    F.write_case(path, flipped, rays)
    got, bits = F.host_step(hostforbes, path)
    assert np.isnan(got[:6, 1]).all() and not np.isnan(got[:, [0, 2]]).any() and bits == 0
    np.testing.assert_array_equal(got[:, 0], got[:, 2])
    # glass to air at a steep angle: total internal reflection
    tir = S.SystemTable.from_json(c["table"].to_json())
    tir.optics["n1"][F.FORBES], tir.optics["n2"][F.FORBES] = 1.8, 1.0
    steep = c["rows"][0][:, :1].copy()
    steep[3:6, 0] = [0.0, np.sin(1.0), np.cos(1.0)]
    steep[1, 0] = steep[2, 0] * np.tan(1.0)   # aimed at the vertex
    F.write_case(path, tir, steep)
    got, bits = F.host_step(hostforbes, path)
    assert bits == S.STATUS_NAN_DIRECTION and np.isnan(got[3:6, 0]).all() \
        and not np.isnan(got[:3, 0]).any()


# ------------------------------------------------------------------ table rules and refusals
def _lines(text):
    out = {}
    for line in text.splitlines():
        what, rest = line.split(": ", 1)
        code, _, msg = rest.partition(" ")
        out[what] = (int(code), msg)
    return out


def test_every_range_walking_entry_refuses_a_forbes_row(hostforbes, tmp_path):
    """OL_EUNSUPPORTED naming the surface, before any launch -- and a range in front of the row
    is an ordinary one."""
    for name in ("q_norm12_default", "q2d_norm12_default"):
        c = F.case(name)
        path = tmp_path / "refuse.case"
        F.write_case(path, c["table"], c["rows"][0][:, :1])
        got = _lines(F.run_host(hostforbes, "refuse", path))
        for who in ("ol_trace", "ol_trace one surface", "ol_trace_ex", "ol_newton_count",
                    "ol_trace_generate", "ol_trace_spot", "ol_trace_spot_batch", "ol_trace_opd",
                    "ol_wavefront_reference", "ol_trace_opd_dev", "ol_aim_rays"):
            assert got[who][0] == -2 and "surface 1 is a Forbes surface" in got[who][1], (who, got[who])
        assert got["ol_trace before the row"] == (0, "ok")


def test_argument_rules_on_a_host_system(hostforbes, tmp_path):
    """ol_trace_forbes's host rules (csrc/forbes_host.h) without a device: each text, and the
    first broken rule answers."""
    c = F.case("q_norm12_default")
    lo, hi = c["sets"]["hex127"]
    path = tmp_path / "rules.case"
    F.write_case(path, c["table"], c["rows"][0][:, lo:hi])
    got = _lines(F.run_host(hostforbes, "rules", path))
    for ok in ("good", "good fp32 midrange", "empty"):
        assert got[ok] == (0, "ok"), ok
    who = "ol_trace_forbes: "
    for what, code, text in (
            ("null system", -1, "system is NULL"), ("dtype", -1, "bad dtype 5"),
            ("negative count", -1, "negative ray count"),
            ("surface -1", -1, "surface -1 outside [0, 4)"),
            ("surface past the table", -1, "surface 4 outside [0, 4)"),
            ("not a forbes row", -1, "surface 2 is not a Forbes surface (geometry kind 1): trace it "
                                     "with ol_trace"),
            ("wavelength", -1, "wavelength index 1 outside [0, 1)"),
            ("wavelength -1", -1, "wavelength index -1 outside [0, 1)"),
            ("flags", -1, "flags 0x4: OL_TRACE_WRITE_RAYS and OL_TRACE_MIDRANGE only"),
            ("too many", -1, "137438953409 rays are more than one launch takes"),
            ("null rays", -1, "rays is NULL"), ("null plane", -1, "rays[5] is NULL"),
            ("stride", -1, "record_stride 126 < n_rays 127"),
            ("nothing to write", -1, "nothing to write (no record_row, no OL_TRACE_WRITE_RAYS)"),
            ("all at once", -1, "bad dtype 5"), ("all but dtype", -1, "negative ray count"),
            ("surface before wavelength", -1, "surface 4 outside [0, 4)"),
            ("wavelength before flags", -1, "wavelength index -1 outside [0, 1)"),
            ("flags before planes", -1, "flags 0xffffffff: OL_TRACE_WRITE_RAYS and "
                                        "OL_TRACE_MIDRANGE only")):
        assert got[what] == (code, who + text), (what, got[what])
    # a polarisation-dependent coating on the row: unpolarised launches only
    coated = S.SystemTable.from_json(c["table"].to_json())
    coated.surfaces["coating_kind"][F.FORBES] = S.COAT_FRESNEL
    F.write_case(path, coated, c["rows"][0][:, lo:hi])
    got = _lines(F.run_host(hostforbes, "rules", path))
    assert got["good"] == (-2, who + "surface 1 carries a polarisation-dependent coating "
                                     "(unpolarised launches only)")
    assert got["flags"][1].startswith(who + "flags 0x4")   # (the flags are looked at first)


def test_system_create_validates_forbes_blocks(hostforbes, tmp_path):
    def create(table):
        path = tmp_path / "create.case"
        F.write_case(path, table, np.zeros((8, 1)))
        return _lines(F.run_host(hostforbes, "create", path))["create"]

    for name in ("q_norm12_default", "q2d_norm12_default"):
        good = F.case(name)["table"]
        assert create(good) == (0, "ok")
        for bad in (0.0, -3.0, np.inf, np.nan):
            t = S.SystemTable.from_json(good.to_json())
            t.surfaces["norm_radius"][F.FORBES] = bad
            code, msg = create(t)
            assert code == -1 and "norm_radius" in msg, (bad, code, msg)
        t = S.SystemTable.from_json(good.to_json())
        t.coeffs[int(t.surfaces["coeff_offset"][F.FORBES]) + 2] = np.nan
        assert create(t)[0] == -1
        t = S.SystemTable.from_json(good.to_json())
        t.surfaces["interaction"][F.FORBES] = S.INTERACT_RECORD_ONLY
        assert create(t)[0] == -2
    good = F.case("q2d_norm12_default")["table"]
    off, n = int(good.surfaces["coeff_offset"][F.FORBES]), int(good.surfaces["n_coeff"][F.FORBES])
    for at, value in ((0, 4.0), (1, 7.0), (0, 2.5), (0, -1.0), (1, 1e9)):   # n0, M
        t = S.SystemTable.from_json(good.to_json())
        t.coeffs[off + at] = value
        code, msg = create(t)
        assert code == -1 and "does not match the counts" in msg, (at, value, code, msg)
    for length in (n - 1, n + 1):
        t = S.SystemTable.from_json(good.to_json())
        t.coeffs = np.concatenate([t.coeffs, np.zeros(4)])
        t.surfaces["n_coeff"][F.FORBES] = length
        assert create(t)[0] == -1


def test_python_layers_know_the_new_kinds():
    from optiland_amd import _capi

    assert (S.GEOM_FORBES_Q, S.GEOM_FORBES_Q2D) == (9, 10) == (_capi.GEOM_FORBES_Q,
                                                              _capi.GEOM_FORBES_Q2D)
    assert "ol_trace_forbes" in _capi.EXPORTS and _capi.ABI_VERSION == 11
    header = open(os.path.join(_live.ROOT, "include", "optiland_hip.h")).read()
    assert "OL_GEOM_FORBES_Q = 9" in header and "OL_GEOM_FORBES_Q2D = 10" in header
    assert "#define OL_ABI_VERSION 11" in header
    for name in ("q_norm12_tight", "q2d_tilted_default"):
        t = F.case(name)["table"]
        again = S.SystemTable.from_json(t.to_json())
        assert again.forbes == (F.FORBES,) == t.forbes
        assert again.to_json() == t.to_json()
        np.testing.assert_array_equal(again.coeffs, t.coeffs)


def test_split_trace_walks_runs_and_rows_in_order():
    from optiland_amd.engine import split_trace

    rec = np.zeros((6, 8, 4))
    calls = []

    def fused(a, b, view, r0, mid):
        calls.append(("fused", a, b, None if view is None else view.shape[0], r0, mid))

    def one(s, row, mid):
        calls.append(("one", s, None if row is None else row.shape, mid))

    split_trace((2, 3, 6), 0, 6, rec[:5], 2, fused, one)
    assert calls == [("fused", 0, 1, None, None, True), ("one", 2, (8, 4), True),
                     ("one", 3, (8, 4), True), ("fused", 4, 5, 3, 4, True),
                     ("one", 6, (8, 4), False)]
    calls.clear()
    split_trace((1,), 0, 3, None, 0, fused, one)
    assert calls == [("fused", 0, 0, None, None, True), ("one", 1, None, True),
                     ("fused", 2, 3, None, None, False)]


def test_trace_dispatches_every_single_kind_in_one_table():
    """One table with all four one-launch kinds (nothing is launched: only `geom_kind` matters):
    the rows each kind owns, and which `trace_<name>` serves which row of a split range."""
    import torch

    from optiland_amd.engine import HipSystem

    kinds = [S.GEOM_PLANE, S.GEOM_FORBES_Q, S.GEOM_STANDARD, S.GEOM_FORBES_Q2D,
             S.GEOM_PLANE_GRATING, S.GEOM_STANDARD_GRATING, S.GEOM_STANDARD, S.GEOM_PLANE_PHASE,
             S.GEOM_GRID_SAG, S.GEOM_PLANE]
    desc = np.zeros(len(kinds), dtype=S.SURFACE_DESC_DTYPE)
    desc["geom_kind"] = kinds
    table = S.SystemTable(surfaces=desc, coeffs=np.zeros(0),
                          optics=np.zeros((len(kinds), 1), dtype=S.SURFACE_OPTICS_DTYPE),
                          wavelengths=np.array([0.55]))
    assert table.forbes == (1, 3) and table.gratings == (4, 5)
    assert table.phases == (7,) and table.grid_sag_rows == (8,)
    assert table.singles == (1, 3, 4, 5, 7, 8)
    assert {i: k.name for i, k in table.single_rows.items()} == {
        1: "forbes", 3: "forbes", 4: "grating", 5: "grating", 7: "phase", 8: "grid_sag"}

    hs = HipSystem.__new__(HipSystem)
    hs.device = torch.device("cpu")
    hs._status = torch.zeros(1, dtype=torch.int32)
    hs.table = table
    calls = []

    def recorder(name):
        def launch(rays, surface, wavelength_index=0, midrange=False, **_):
            calls.append((name, surface, midrange))
        return launch

    for name in ("forbes", "grating", "phase", "grid_sag"):
        setattr(hs, "trace_" + name, recorder(name))

    def fused(rays, wavelength_index=0, first=0, last=None, _status_to=None, **_):
        # (`_trace_split` gives a fused run a status word of its own exactly when it is midrange)
        calls.append(("fused", first, last, _status_to is not None))

    hs.trace = fused
    planes = [torch.zeros(3, dtype=torch.float64) for _ in range(8)]
    HipSystem.trace(hs, planes, first=0, last=9, record=False)
    assert calls == [("fused", 0, 0, True), ("forbes", 1, True), ("fused", 2, 2, True),
                     ("forbes", 3, True), ("grating", 4, True), ("grating", 5, True),
                     ("fused", 6, 6, True), ("phase", 7, True), ("grid_sag", 8, True),
                     ("fused", 9, 9, False)]
    with pytest.raises(ValueError):
        HipSystem.trace(hs, planes, first=0, last=9, record=False,
                        prt=torch.zeros((9, 3), dtype=torch.float64))


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
@pytest.mark.parametrize("kind", F.KINDS)
def test_packer_tolerate_packs_the_documented_block(ref, kind):
    from optiland.geometries.forbes import qpoly as Q
    from optiland_amd.packer import UnsupportedSystem, pack_optic, pack_surfaces

    lens = F.singlet(kind, "norm8", 1e-9)
    t = F.packed(lens)
    assert t.forbes == (F.FORBES,) and t.unsupported == ()
    row = t.surfaces[F.FORBES]
    assert int(row["geom_kind"]) == (S.GEOM_FORBES_Q if kind == "q" else S.GEOM_FORBES_Q2D)
    assert (float(row["radius"]), float(row["conic"]), float(row["norm_radius"]),
            float(row["tol"]), int(row["max_iter"])) == (40.0, -0.5, 8.0, 1e-9, 100)
    assert int(row["interaction"]) == S.INTERACT_REFRACT and int(row["aperture_kind"]) == S.AP_NONE
    assert abs(float(t.optics[F.FORBES, 0]["n2"]) - 1.5185) < 1e-3
    block = t.coeffs[int(row["coeff_offset"]):int(row["coeff_offset"]) + int(row["n_coeff"])]
    pn = np.asarray(Q.change_basis_qbfs_to_pn(
        [F.Q_TERMS[n] for n in range(5)] if kind == "q" else
        [F.Q2D_TERMS[("a", 0, n)] for n in range(3)]), dtype=np.float64)
    if kind == "q":
        np.testing.assert_array_equal(block, pn)
    else:
        assert (block[0], block[1]) == (3.0, 3.0)
        np.testing.assert_array_equal(block[2:5], pn)
        at, counts = 5, []
        for m in (1, 2, 3):
            na, nb = int(block[at]), int(block[at + 1])
            counts.append((na, nb))
            quads = block[at + 2:at + 2 + 4 * (na + nb)].reshape(-1, 4)
            if m == 1:   # four a-coefficients: the alpha_3 rule is exercised
                d = np.asarray(Q.change_basis_q2d_to_pnm(
                    [F.Q2D_TERMS[("a", 1, n)] for n in range(4)], 1), dtype=np.float64)
                np.testing.assert_array_equal(quads[:4, 0], d)
                for n in range(3):
                    a, b, _ = Q.abc_q2d_clenshaw(n, 1)
                    assert (quads[n, 1], quads[n, 2]) == (a, b)
                assert quads[0, 3] == Q.abc_q2d_clenshaw(1, 1)[2] and quads[1, 3] == Q.abc_q2d_clenshaw(2, 1)[2]
                assert tuple(quads[3, 1:]) == (0.0, 0.0, 0.0) and quads[2, 3] == 0.0
            at += 2 + 4 * (na + nb)
        assert counts == [(4, 1), (1, 2), (2, 0)] and at == block.size
    # strict packing keeps raising -- also after a tolerant pack filled a cache
    with pytest.raises(UnsupportedSystem):
        pack_optic(lens, wavelengths=[F.WAVELENGTH])
    with pytest.raises(UnsupportedSystem):
        pack_surfaces(lens.surfaces.surfaces, [F.WAVELENGTH])


@needs_reference
def test_packer_strict_after_tolerant_with_a_shared_cache(ref):
    from optiland_amd import fingerprint as fp
    from optiland_amd.packer import UnsupportedSystem, pack_surfaces

    lens = F.singlet("q", "norm12")
    cache: dict = {}
    tok, keep = fp.surfaces_token(lens.surfaces.surfaces, F.WAVELENGTH)
    t = pack_surfaces(lens.surfaces.surfaces, [F.WAVELENGTH], tolerate=True, tokens=tok[1],
                      cache=cache, keep=keep)
    assert t.forbes == (F.FORBES,)
    with pytest.raises(UnsupportedSystem):
        pack_surfaces(lens.surfaces.surfaces, [F.WAVELENGTH], tokens=tok[1], cache=cache, keep=keep)
    again = pack_surfaces(lens.surfaces.surfaces, [F.WAVELENGTH], tolerate=True, tokens=tok[1],
                          cache=cache, keep=keep)
    assert again.to_json() == t.to_json()


@needs_reference
def test_fixture_tables_are_what_the_packer_produces_today(ref):
    for name in F.case_names():
        c = F.case(name)
        lens = F.singlet(c["kind"], c["variant"], c["tol"])
        assert F.packed(lens).to_json() == c["table"].to_json(), name


@needs_reference
def test_packer_leaves_these_to_the_reference(ref):
    """A class merely NAMED like a Forbes geometry, a Jones coating on the surface, the opt-in
    reference Newton rule and a term dictionary the packer cannot read."""
    from optiland.coatings import FresnelCoating
    from optiland.samples.objectives import CookeTriplet

    lens = CookeTriplet()
    g = lens.surfaces[3].geometry
    g.__class__ = type("ForbesQbfsGeometry", (g.__class__,), {})
    t = F.packed(lens)
    assert t.forbes == () and t.unsupported == (3,)

    lens = F.singlet("q2d", "norm12")
    surf = lens.surfaces.surfaces[F.FORBES]
    surf.interaction_model.coating = FresnelCoating(surf.material_pre, surf.material_post)
    t = F.packed(lens)
    assert t.forbes == () and t.unsupported == (F.FORBES,)

    lens = F.singlet("q", "norm12")
    S.OPTIONS["reference_newton"] = True
    try:
        t = F.packed(lens)
    finally:
        S.OPTIONS["reference_newton"] = False
    assert t.forbes == () and t.unsupported == (F.FORBES,)

    lens = F.singlet("q", "norm12")
    lens.surfaces.surfaces[F.FORBES].geometry.radial_terms["two"] = 1e-4
    t = F.packed(lens)
    assert t.forbes == () and t.unsupported == (F.FORBES,)
    lens = F.singlet("q2d", "norm12")
    lens.surfaces.surfaces[F.FORBES].geometry.freeform_coeffs[("c", 1, 1)] = 1e-4
    t = F.packed(lens)
    assert t.forbes == () and t.unsupported == (F.FORBES,)


@needs_reference
@pytest.mark.parametrize("native", [True, False])
def test_surface_token_sees_every_forbes_edit(ref, native):
    from optiland_amd import fingerprint as fp

    was = fp.use_native(native)
    if native and not was:
        fp.use_native(True)
        pytest.skip("native change-detector walk not built")
    try:
        def token(lens):
            tok, _keep = fp.surfaces_token(lens.surfaces.surfaces, F.WAVELENGTH)
            return tok[1][F.FORBES]

        def edits(kind):
            yield "tol", lambda g: setattr(g, "tol", 1e-9)
            yield "max_iter", lambda g: setattr(g, "max_iter", 37)
            yield "norm_radius", lambda g: setattr(g, "norm_radius", ref.array(11.0))
            if kind == "q":
                yield "radial_terms[2]", lambda g: g.radial_terms.__setitem__(2, 3e-4)
                yield "radial_terms[7] (new)", lambda g: g.radial_terms.__setitem__(7, 1e-6)
            else:
                def one(g):
                    g.freeform_coeffs[("a", 1, 2)] = 5e-4
                    g._prepare_coeffs()
                yield "freeform_coeffs[a, 1, 2]", one
                yield "freeform_coeffs alone", \
                    lambda g: g.freeform_coeffs.__setitem__(("b", 2, 1), 1e-4)

        for kind in F.KINDS:
            for what, edit in edits(kind):
                lens = F.singlet(kind, "norm12")
                before = token(lens)
                assert before == token(lens), what
                edit(lens.surfaces.surfaces[F.FORBES].geometry)
                assert before != token(lens), (kind, what)
            # the automatic normalisation (update_normalization: norm_radius None at construction)
            lens = F.singlet(kind, "norm12")
            g = lens.surfaces.surfaces[F.FORBES].geometry
            g.normalization_mode = "auto"
            before = token(lens)
            g.update_normalization(9.5)
            assert before != token(lens), (kind, "update_normalization")
    finally:
        fp.use_native(True)


# ------------------------------------------------------------------ the drop-in, end to end on CPU
@pytest.fixture()
def forbes_on_cpu(ref, monkeypatch, hostforbes, tmp_path):
    import optiland_amd.tracer as tr

    cls = F.make_engine_class(hostforbes, tmp_path)
    cls.forbes_launches = 0
    monkeypatch.setattr(tr, "_make_engine", lambda table, device: cls(table, device))
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


def _numpy_rows(be, kind, variant, tol, edit=None):
    be.set_backend("numpy")
    try:
        lens = F.singlet(kind, variant, tol)
        if edit is not None:
            edit(lens.surfaces.surfaces[F.FORBES].geometry)
        lens.trace(0.0, 1.0, F.WAVELENGTH, 6, "hexapolar")
        return _recorded(be, lens)
    finally:
        be.set_backend("torch")
        be.set_device("cpu")
        be.set_precision("float64")


@needs_reference
@pytest.mark.parametrize("kind", F.KINDS)
def test_dropin_traces_the_forbes_surface_on_the_engine(forbes_on_cpu, kind):
    (be, cls) = forbes_on_cpu
    from optiland_amd import integration as I

    c = F.case(f"{kind}_norm12_tight")
    lo, hi = c["sets"]["hex127"]
    lens = F.singlet(kind, "norm12", F.TIGHT)
    tracer = I.install(lens, force=True)
    foreign, served = I._SG["foreign"], I._SG["count"]
    rays = lens.trace(0.0, 1.0, F.WAVELENGTH, 6, "hexapolar")
    assert tracer.last_path == "reference"       # strict packing still declines the optic ...
    assert I._SG["count"] == served + 1          # ... its SurfaceGroup.trace is the bridge's
    assert I._SG["foreign"] == foreign           # and no surface went to the reference's own trace
    assert cls.forbes_launches == 1
    got = _recorded(be, lens)
    assert got.shape == (4, 8, 127) and not np.isnan(got).any()   # every recorded array is filled
    F.compare(got, c, np.float64, lo, hi, report=print)
    np.testing.assert_array_equal(np.asarray(be.to_numpy(rays.x)), got[3, 0])

    # an edit between two traces shows as the reference's does: one coefficient, then norm_radius
    geom = lens.surfaces.surfaces[F.FORBES].geometry

    def coefficient(g):
        if kind == "q":
            g.radial_terms[2] = be.array(4e-4) if be.get_backend() == "torch" else 4e-4
        else:
            g.freeform_coeffs[("a", 1, 2)] = be.array(4e-4) if be.get_backend() == "torch" else 4e-4
        g._prepare_coeffs()

    def norm_radius(g):
        coefficient(g)
        g.norm_radius = be.array(10.5)

    before = got
    for edit in (coefficient, norm_radius):
        edit(geom)
        lens.trace(0.0, 1.0, F.WAVELENGTH, 6, "hexapolar")
        got = _recorded(be, lens)
        want = _numpy_rows(be, kind, "norm12", F.TIGHT, edit)
        assert np.abs(got[3, :2] - before[3, :2]).max() > 1e-6     # the edit is visible ...
        edited = dict(c, rows=want, edge=np.zeros(127, dtype=bool), name=f"{kind} {edit.__name__}")
        F.compare(got, edited, np.float64, report=print)           # ... and is the reference's
        before = got
    assert I._SG["foreign"] == foreign and cls.forbes_launches == 3


@needs_reference
def test_dropin_polarised_bundle_takes_the_references_surface(forbes_on_cpu):
    (be, cls) = forbes_on_cpu
    from optiland.rays import PolarizationState
    from optiland_amd import integration as I

    lens = F.singlet("q", "norm12", F.TIGHT)
    lens.updater.set_polarization(PolarizationState(is_polarized=False))
    I.install(lens, force=True)
    foreign = I._SG["foreign"]
    lens.trace(0.0, 1.0, F.WAVELENGTH, 6, "hexapolar")
    assert cls.forbes_launches == 0 and I._SG["foreign"] == foreign + 1
    got = _recorded(be, lens)
    c = F.case("q_norm12_tight")
    lo, hi = c["sets"]["hex127"]
    F.compare(got[:, :6], dict(c, rows=c["rows"][:, :6], spread=c["spread"][:, :6],
                               gap=c["gap"][:, :6]), np.float64, lo, hi)
