"""Phase-profile surfaces without a GPU: the host build of optiland_amd/csrc/phase_device.h
(tests/hostphase) against the fixture tests/golden/phase.npz and the reference's own known
answers, the rules of ol_trace_phase and of ol_system_create, the refusal of every range-walking
entry point, the packer, the change detector and the drop-in end to end on CPU tensors.  Bounds
and fixture: tests/_phase.py.
"""

from __future__ import annotations

import math
import os
import subprocess
import sys

import numpy as np
import pytest

from optiland_amd import system as S
from tests import _live
from tests import _phase as P

REF = _live.reference_root() or _live.STAGED
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "optiland")),
                                     reason="reference package not present")
G = P.PHASE


@pytest.fixture(scope="module")
def hostphase():
    b = P._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return b.build()


# ------------------------------------------------------------------ the fixture itself
def test_fixture_holds_the_cases_and_keeps_its_margins():
    """Every case of the issue is there; no ray has |S| / n2'^2 < 1e-2 or lies within 1e-4 of a
    pitch of a grid line, and at most 1 % of a case's rays went at grid lines; the TIR cases have
    between 10 % and 90 % clipped rays with finite directions, the others no evanescent ray; the
    clipped case clips some rays; the grid case has hits inside the grid, within one cell outside
    it and further out; the 1027-ray set is in two cases only; all four profile kinds occur."""
    assert set(P.case_names()) == set(P.CASES)
    big = [n for n in P.case_names() if "big_in" in P.case(n)]
    assert sorted(big) == sorted(P.BIG_CASES)
    kinds = set()
    for name in P.case_names():
        c = P.case(name)
        g, wl, rows, table = c["g"], c["wl"], c["rows"], c["table"]
        assert g == G and table.phases == (g,) and wl == P.CASES[name][3]
        block = P.block_of(table, g)
        kinds.add(int(block[0]))
        pairs = [(rows[g - 1], rows[g])]
        if name in P.BIG_CASES:
            pairs.append((c["big_in"], c["big_out"]))
            assert 900 < c["big_in"].shape[1] <= 1027
        assert 100 < rows.shape[2] <= 127
        assert int(c["dropped"][1]) <= P.GRID_DROP_CAP * 127
        assert rows.shape[2] == 127 - int(c["dropped"].sum())
        for before, after in pairs:
            s = P.radicand(table, g, before, after, wl)
            assert np.abs(s).min() >= P.MARGIN, (name, float(np.abs(s).min()))
            d = P.grid_line_distance(block, *P.local_hit(table, g, after))
            assert d.min() >= P.GRID_MARGIN, (name, float(d.min()))
            assert not np.isnan(after).any(), name
            tir = s < 0
            assert np.all(after[6][tir] == 0.0), name
            if name in P.TIR_CASES:
                assert 0.1 <= tir.mean() <= 0.9, (name, float(tir.mean()))
                assert np.array_equal(after[6] == 0.0, tir), name
            else:
                assert not tir.any(), name
        if name == "clipped":
            assert 0 < (rows[g, 6] == 0).sum() < rows.shape[2]
        if name == "grid":
            ix, iy = P.grid_coordinates(block, *P.local_hit(table, g, rows[g]))
            far = np.maximum(np.maximum(-ix, ix - (block[2] - 1)),
                             np.maximum(-iy, iy - (block[3] - 1)))
            assert ((far > 0) & (far < 1)).any() and (far > 1).any() and (far < 0).any()
    assert kinds == {S.PHASE_CONSTANT, S.PHASE_LINEAR, S.PHASE_RADIAL, S.PHASE_GRID}
    assert len({P.CASES[n][2] for n in P.CASES}) >= 2           # at least two fields
    assert os.path.getsize(P.GOLD) < 400_000


# ------------------------------------------------------------------ host build against the fixture
def _host_case(exe, tmp_path, c, before, want, what, report=print):
    scale = P.scale_of(c["rows"][:c["g"] + 1])
    worst = {}
    for dtype in (np.float64, np.float32):
        path = tmp_path / "step.case"
        P.write_case(path, c["table"], before, c["g"], fp64=dtype is np.float64, wl_index=c["wl"])
        got, bits = P.host_step(exe, path)
        assert bits == 0        # an evanescent ray keeps a finite direction: no status bit
        worst[dtype] = P.compare(got, want, dtype, scale, what, report=report)
        if dtype is np.float64:
            P.compare(got, want, dtype, scale, what, tight=True, report=report)
    return worst


@pytest.mark.parametrize("name", list(P.CASES))
def test_host_step_against_every_case(hostphase, tmp_path, name):
    """The one-surface step, fp64 and fp32: the phase plane's recorded row from the row in front
    of it, within the contract -- and fp64 within 1e-12; NaN and i == 0 masks equal."""
    c = P.case(name)
    g = c["g"]
    _host_case(hostphase, tmp_path, c, c["rows"][g - 1], c["rows"][g], name)
    if name in P.BIG_CASES:
        _host_case(hostphase, tmp_path, c, c["big_in"], c["big_out"], name + " " + P.BIG_SET)


def test_host_step_gives_the_references_known_answers(hostphase, tmp_path):
    """The constants of the reference's tests/test_phase_interaction_model.py and
    tests/test_radial_phase.py out of the packed single-surface step, to those files' own
    tolerances, and what the reference itself traced to 1e-12."""
    gd = P.golden()
    n = gd["known_in"].shape[0]
    assert n == 10 and gd["known_out"].shape == (n, 8)
    q = 0.5 * 1e-3 / (2 * math.pi)
    seen = set()
    for k in range(n):
        what, want = str(gd["known_what"][k]), float(gd["known_want"][k])
        table = S.SystemTable.from_json(str(gd["known_table"][k]))
        assert table.phases == (G,) and float(table.wavelengths[0]) == 0.5
        path = tmp_path / "known.case"
        P.write_case(path, table, gd["known_in"][k][:, None], G)
        got, bits = P.host_step(hostphase, path)
        got = got[:, 0]
        x, y = gd["known_in"][k][:2]
        print(f"known answer {k} ({what}): {got.tolist()}")
        assert bits == 0
        if what == "L":
            np.testing.assert_allclose(got[3:5], [want, 0.0], rtol=0, atol=1e-6)
            assert want == -1.0 / 150.0
        elif what == "N<0":
            assert got[5] < 0
        elif what == "i=0":
            assert got[6] == 0.0 and np.isfinite(got[3:6]).all()
        elif what == "phi":
            np.testing.assert_allclose(-got[7] / q, want, rtol=1e-7, atol=1e-9)
        else:
            np.testing.assert_allclose(got[3:5] * 1.5 / q, [x, y], rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(got, gd["known_out"][k], rtol=0, atol=1e-12 * 40)
        seen.add(what)
    assert seen == {"L", "N<0", "i=0", "phi", "grad"}


def test_host_step_under_the_sanitizers(tmp_path):
    """The same program built with AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone
    program: the runtime is linked into it) runs the same cases clean, a NaN and a far-away
    position on the grid row (no read outside the block), and its other modes."""
    b = P._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    if not P.sanitizers_available(tmp_path):
        pytest.skip("this box cannot build or run a sanitized program at all")
    exe = b.build(sanitize=True)     # (a failure to build the checker is a failure)
    for name in P.CASES:
        c = P.case(name)
        g = c["g"]
        _host_case(exe, tmp_path, c, c["rows"][g - 1], c["rows"][g], name, report=None)
    for name in ("grid", "height_blue"):
        _nan_position_on_a_grid_row(exe, tmp_path, name)
    path = tmp_path / "step.case"
    assert "ol_trace: -2" in P.run_host(exe, "refuse", path)
    assert "good: 0 ok" in P.run_host(exe, "rules", path)
    assert "create: 0 ok" in P.run_host(exe, "create", path)


def _nan_position_on_a_grid_row(exe, tmp_path, name):
    """Rays whose position is NaN, infinite or astronomically far from the grid, between two
    ordinary ones: NaN (or, far away, the plain refraction of a zero phase) for them, their
    neighbours untouched, in both precisions."""
    c = P.case(name)
    g = c["g"]
    good = c["rows"][g - 1][:, :1]
    rays = np.repeat(good, 7, axis=1)
    rays[0, 1] = np.nan
    rays[1, 2] = np.nan
    rays[0, 3] = 1e300
    rays[1, 4] = -1e30
    rays[0, 5], rays[1, 5] = np.inf, -np.inf
    for fp64 in (True, False):
        path = tmp_path / "nan.case"
        P.write_case(path, c["table"], rays, g, fp64=fp64, wl_index=c["wl"])
        got, bits = P.host_step(exe, path)
        # (a NaN y alone leaves x finite: a position without a direction, the bit's meaning)
        assert bits == S.STATUS_NAN_DIRECTION
        np.testing.assert_array_equal(got[:, 0], got[:, 6])
        assert np.isfinite(got[:, 0]).all()
        for k in (1, 2):   # a NaN position: NaN direction and path
            assert np.isnan(got[3:6, k]).all() and np.isnan(got[7, k]), (name, k, got[:, k])
        for k in (3, 4):   # far outside the grid: every neighbour masked, phase 0, gradient 0
            if fp64:
                assert np.isfinite(got[3:6, k]).all(), (name, k, got[:, k])
        assert not np.isfinite(got[3:6, 5]).all()


def test_host_nan_neighbours_a_miss_and_the_axis(hostphase, tmp_path):
    """NaN neighbours on a grid row (`_nan_position_on_a_grid_row`); a ray with N = 0 never
    reaches the plane: nothing finite comes back for it and its neighbours are untouched; a ray
    along the axis of the radial row (r = 0) gets no transverse part at all, no 0 / 0."""
    _nan_position_on_a_grid_row(hostphase, tmp_path, "grid")
    _nan_position_on_a_grid_row(hostphase, tmp_path, "height")
    c = P.case("radial_t")
    g = c["g"]
    good = c["rows"][g - 1][:, :1]
    rays = np.repeat(good, 3, axis=1)
    rays[3:6, 1] = (1.0, 0.0, 0.0)
    path = tmp_path / "miss.case"
    P.write_case(path, c["table"], rays, g)
    got, bits = P.host_step(hostphase, path)
    assert not np.isfinite(got[:3, 1]).any()
    np.testing.assert_array_equal(got[:, 0], got[:, 2])
    assert np.isfinite(got[:, 0]).all()
    for name, nz in (("radial_t", 1.0), ("radial_r", -1.0), ("radial_air", 1.0)):
        c = P.case(name)
        z0 = float(c["rows"][g - 1][2, 0])
        axis = np.array([[0.0], [0.0], [z0], [0.0], [0.0], [1.0], [1.0], [0.25]])
        for fp64 in (True, False):
            P.write_case(path, c["table"], axis, g, fp64=fp64)
            got, bits = P.host_step(hostphase, path)
            np.testing.assert_array_equal(got[3:5, 0], [0.0, 0.0])
            assert abs(got[5, 0] - nz) <= (4 * 2.3e-16 if fp64 else 4 * 1.2e-7)   # kz / |kz|
            assert got[0, 0] == 0.0 and got[1, 0] == 0.0 and got[6, 0] == 1.0
            assert abs(got[7, 0] - (0.25 + 5.0)) <= 1e-5     # the path to the plane, phase 0


# ------------------------------------------------------------------ rules and refusals
def _lines(text):
    out = {}
    for line in text.splitlines():
        what, rest = line.split(": ", 1)
        code, _, msg = rest.partition(" ")
        out[what] = (int(code), msg)
    return out


def test_every_range_walking_entry_refuses_a_phase_row(hostphase, tmp_path):
    """OL_EUNSUPPORTED naming the surface, before any launch -- and a range in front of the row
    is an ordinary one."""
    for name in ("radial_t", "grid", "linear_m1", "constant"):
        c = P.case(name)
        path = tmp_path / "refuse.case"
        P.write_case(path, c["table"], c["rows"][0][:, :1], c["g"])
        got = _lines(P.run_host(hostphase, "refuse", path))
        for who in ("ol_trace", "ol_trace one surface", "ol_trace_ex", "ol_newton_count",
                    "ol_trace_generate", "ol_trace_spot", "ol_trace_spot_batch", "ol_trace_opd",
                    "ol_wavefront_reference", "ol_trace_opd_dev", "ol_aim_rays"):
            assert got[who][0] == -2 and "surface 2 is a phase surface" in got[who][1], \
                (who, got[who])
        assert got["ol_trace"][1] == ("ol_trace: surface 2 is a phase surface: trace it with "
                                      "ol_trace_phase and cut the range there")
        assert got["ol_trace before the row"] == (0, "ok")


def test_argument_rules_on_a_host_system(hostphase, tmp_path):
    """ol_trace_phase's host rules (csrc/phase_host.h) without a device: each text, and the first
    broken rule answers -- the rules and the order of ol_trace_grating."""
    c = P.case("radial_t")
    path = tmp_path / "rules.case"
    P.write_case(path, c["table"], c["rows"][0], c["g"])
    got = _lines(P.run_host(hostphase, "rules", path))
    for ok in ("good", "good fp32 midrange", "empty"):
        assert got[ok] == (0, "ok"), ok
    who = "ol_trace_phase: "
    um = "must be finite and greater than 0"
    for what, code, text in (
            ("null system", -1, "system is NULL"), ("dtype", -1, "bad dtype 5"),
            ("negative count", -1, "negative ray count"),
            ("surface -1", -1, "surface -1 outside [0, 4)"),
            ("surface past the table", -1, "surface 4 outside [0, 4)"),
            ("not a phase row", -1, "surface 3 is not a phase surface (geometry kind 0): trace "
                                    "it with ol_trace"),
            ("wavelength", -1, "wavelength index 1 outside [0, 1)"),
            ("wavelength -1", -1, "wavelength index -1 outside [0, 1)"),
            ("wavelength_um 0", -1, f"wavelength_um 0 {um}"),
            ("wavelength_um negative", -1, f"wavelength_um -0.5 {um}"),
            ("wavelength_um inf", -1, f"wavelength_um inf {um}"),
            ("flags", -1, "flags 0x4: OL_TRACE_WRITE_RAYS and OL_TRACE_MIDRANGE only"),
            ("too many", -1, "137438953409 rays are more than one launch takes"),
            ("null rays", -1, "rays is NULL"), ("null plane", -1, "rays[5] is NULL"),
            ("stride", -1, "record_stride 126 < n_rays 127"),
            ("nothing to write", -1, "nothing to write (no record_row, no OL_TRACE_WRITE_RAYS)"),
            ("all at once", -1, "bad dtype 5"), ("all but dtype", -1, "negative ray count"),
            ("surface before wavelength", -1, "surface 4 outside [0, 4)"),
            ("wavelength index before wavelength_um", -1, "wavelength index -1 outside [0, 1)"),
            ("wavelength_um before flags", -1, f"wavelength_um 0 {um}"),
            ("flags before planes", -1, "flags 0xffffffff: OL_TRACE_WRITE_RAYS and "
                                        "OL_TRACE_MIDRANGE only")):
        assert got[what] == (code, who + text), (what, got[what])
    assert got["wavelength_um nan"][0] == -1 and um in got["wavelength_um nan"][1]
    coated = S.SystemTable.from_json(c["table"].to_json())
    coated.surfaces["coating_kind"][c["g"]] = S.COAT_FRESNEL
    P.write_case(path, coated, c["rows"][0], c["g"])
    got = _lines(P.run_host(hostphase, "rules", path))
    assert got["good"] == (-2, who + "surface 2 carries a polarisation-dependent coating "
                                     "(unpolarised launches only)")


def _edited(table, g, edit, n_coeff=None):
    """A copy of `table` whose phase block (the LAST block of the coefficient buffer in every
    fixture table) went through `edit(block) -> block`."""
    t = S.SystemTable.from_json(table.to_json())
    off, n = int(t.surfaces["coeff_offset"][g]), int(t.surfaces["n_coeff"][g])
    assert off + n == t.coeffs.size
    block = np.asarray(edit(t.coeffs[off:off + n].copy()), dtype=np.float64)
    # (a shorter block leaves the buffer its length: later rows keep their offsets inside it)
    t.coeffs = np.concatenate([t.coeffs[:off], block, np.zeros(max(0, n - block.size))])
    t.surfaces["n_coeff"][g] = block.size if n_coeff is None else n_coeff
    return t


def test_system_create_validates_phase_blocks(hostphase, tmp_path):
    """Every rule of the block, each answered with OL_EINVAL and a text that names the surface
    and the rule; the good blocks of all four kinds are taken."""
    def create(table):
        path = tmp_path / "create.case"
        P.write_case(path, table, np.zeros((8, 1)), G)
        return _lines(P.run_host(hostphase, "create", path))["create"]

    def put(at, value):
        def edit(b):
            b[at] = value
            return b
        return edit

    def refused(table, *words):
        code, msg = create(table)
        assert code == -1 and msg.startswith("surface 2: ") and all(w in msg for w in words), \
            (words, code, msg)

    tables = {k: P.case(n)["table"] for k, n in (("constant", "constant"), ("linear", "linear_m1"),
                                                ("radial", "radial_t"), ("grid", "grid"),
                                                ("height", "height"))}
    for t in tables.values():
        assert create(t) == (0, "ok")
    for t in tables.values():
        # the kind is one of the four, whole; the efficiency is finite
        for bad in (4.0, -1.0, 1.5, np.nan, np.inf):
            refused(_edited(t, G, put(0, bad)), "phase profile kind")
        for bad in (np.nan, np.inf, -np.inf):
            refused(_edited(t, G, put(1, bad)), "efficiency", "finite")
        refused(_edited(t, G, lambda b: b[:1]), "phase profile kind")
    # counts add up to n_coeff exactly
    refused(_edited(tables["constant"], G, lambda b: np.append(b, 0.0)), "constant", "3 values")
    refused(_edited(tables["constant"], G, lambda b: b[:2]), "constant", "3 values")
    refused(_edited(tables["linear"], G, lambda b: b[:3]), "linear", "4 values")
    refused(_edited(tables["linear"], G, lambda b: np.append(b, 0.0)), "linear", "4 values")
    for bad in (2.0, 4.0, 2.5, -1.0, np.nan, 1e9):
        refused(_edited(tables["radial"], G, put(2, bad)), "radial", "term count")
    refused(_edited(tables["radial"], G, lambda b: b[:-1]), "radial", "term count")
    refused(_edited(tables["radial"], G, lambda b: np.append(b, 1.0)), "radial", "term count")
    empty = _edited(tables["radial"], G, lambda b: np.array([2.0, 1.0, 0.0]))
    assert create(empty) == (0, "ok")                       # no terms: a plain refraction
    for name in ("grid", "height"):
        t = tables[name]
        for at in (2, 3):       # W, H >= 2 and whole
            for bad in (1.0, 0.0, -3.0, 2.5, np.nan, np.inf):
                refused(_edited(t, G, put(at, bad)), "W, H >= 2")
        for at in (4, 5, 6, 7):  # the four bounds are finite
            for bad in (np.nan, np.inf, -np.inf):
                refused(_edited(t, G, put(at, bad)), "bound", "not finite")
        refused(_edited(t, G, lambda b: put(5, b[4])(b)), "bounds coincide")
        refused(_edited(t, G, lambda b: put(7, b[6])(b)), "bounds coincide")
        # n_scale is 0 or the wavelength count (1 for the grid case, 2 for the height case)
        for bad in (3.0, 0.5, -1.0, np.nan):
            refused(_edited(t, G, put(8, bad)), "scale count")
        refused(_edited(t, G, lambda b: b[:-1]), "does not match the counts")
        refused(_edited(t, G, lambda b: np.append(b, 0.0)), "does not match the counts")
        refused(_edited(t, G, put(2, 23.0)), "does not match the counts")
        refused(_edited(t, G, lambda b: b[:8]), "W, H >= 2")
    refused(_edited(tables["grid"], G, put(8, 1.0)), "does not match the counts")
    refused(_edited(tables["height"], G, put(8, 1.0)), "scale count", "wavelength count 2")
    refused(_edited(tables["height"], G, put(8, 0.0)), "does not match the counts")
    # a block that runs past the buffer, a surface that only records
    t = S.SystemTable.from_json(tables["radial"].to_json())
    t.surfaces["n_coeff"][G] += 1
    assert create(t)[0] == -1 and "exceeds the buffer" in create(t)[1]
    t = S.SystemTable.from_json(tables["radial"].to_json())
    t.surfaces["interaction"][G] = S.INTERACT_RECORD_ONLY
    assert create(t) == (-2, "surface 2: a phase surface that only records")
    # the kind behind the last one is refused with the text it always had
    t = S.SystemTable.from_json(tables["radial"].to_json())
    t.surfaces["geom_kind"][G] = 15
    assert create(t) == (-2, "surface 2: geometry kind 15")
    t.surfaces["geom_kind"][G] = 13     # (never a kind: refused as before the phase kind came)
    assert create(t) == (-2, "surface 2: geometry kind 13")


def test_python_layers_know_the_new_kind_and_the_library_exports_the_entry():
    from optiland_amd import _capi, build

    assert S.GEOM_PLANE_PHASE == 14 == _capi.GEOM_PLANE_PHASE
    assert S.GEOM_NAMES[14] == "plane_phase" and 13 not in S.GEOM_NAMES
    assert (S.PHASE_CONSTANT, S.PHASE_LINEAR, S.PHASE_RADIAL, S.PHASE_GRID) == (0, 1, 2, 3)
    assert "ol_trace_phase" in _capi.EXPORTS and _capi.ABI_VERSION == 11
    header = open(os.path.join(_live.ROOT, "include", "optiland_hip.h")).read()
    assert "OL_GEOM_PLANE_PHASE = 14" in header and "int ol_trace_phase(" in header
    assert "#define OL_ABI_VERSION 11" in header
    build.build_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.library_path()], text=True)
    assert " T ol_trace_phase" in out
    lib = _capi.load()
    assert _capi.has_trace_phase(lib) and lib.ol_abi_version() == 11
    for name in ("radial_t", "grid", "height"):
        t = P.case(name)["table"]
        again = S.SystemTable.from_json(t.to_json())
        assert again.phases == (G,) == t.phases and again.forbes == () and again.gratings == ()
        assert again.to_json() == t.to_json()
        assert again.reference_newton_surfaces() == []


def test_built_library_answers_the_host_rules_without_a_device():
    """The product library, not the checker: the rules of ol_trace_phase that need no system come
    back before anything touches a device."""
    from optiland_amd import _capi, build

    build.build_library()
    lib = _capi.load()
    rc = lib.ol_trace_phase(None, _capi.F64, 1, None, 0, 0.587, None, 0, 1, 1, None, None)
    assert rc == -1 and lib.ol_last_error() == b"ol_trace_phase: system is NULL"


def test_engine_and_tracer_declare_the_capability():
    import optiland_amd.tracer as tr
    from optiland_amd.engine import HipSystem

    assert tr._make_engine.traces_phases is True and tr._make_engine.traces_gratings is True
    assert callable(HipSystem.can_trace_phase) and callable(HipSystem.trace_phase)


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


def _torch64(be):
    be.set_backend("torch")
    be.set_device("cpu")
    be.set_precision("float64")


@needs_reference
def test_packer_packs_the_documented_row_and_block(ref):
    """The row and the block of each of the five profiles; the fixture's tables are today's."""
    from optiland_amd.packer import UnsupportedSystem, pack_optic, pack_surfaces

    xs, ys = P.grid_axes()
    nodes = P.radial_phase(xs[None, :], ys[:, None])
    k = 2 * math.pi / 5.0e-3
    want = {
        "radial_t": [2.0, 1.0, 3.0, *P.RADIAL],
        "linear_m1": [1.0, 0.8, -k * math.cos(0.6), -k * math.sin(0.6)],
        "constant": [0.0, 1.0, 1.3],
        "grid": [3.0, 1.0, 24.0, 18.0, -2.6, 2.4, -2.2, 2.5, 0.0, *nodes.reshape(-1)],
    }
    try:
        for name in ("radial_t", "linear_m1", "constant", "grid", "height", "tilted",
                     "radial_r"):
            if name in P.TORCH_CASES:
                _torch64(ref)
            else:
                ref.set_backend("numpy")
            lens = P.case_lens(name)
            t = P.packed(lens, P.case_wavelengths(name))
            assert t.phases == (G,) and t.unsupported == () and t.forbes == () == t.gratings
            row = t.surfaces[G]
            assert int(row["geom_kind"]) == S.GEOM_PLANE_PHASE
            block = P.block_of(t, G)
            if name in want:
                np.testing.assert_allclose(block, want[name], rtol=1e-15, atol=0)
            if name == "height":
                assert block[:9].tolist() == [3.0, 1.0, 24.0, 18.0, -2.6, 2.4, -2.2, 2.5, 2.0]
                n = [float(np.asarray(ref.to_numpy(lens.surfaces.surfaces[G].interaction_model
                                                   .phase_profile.material.n(w))).reshape(-1)[0])
                     for w in P.WAVELENGTHS]
                scales = [2 * math.pi / (w * 1e-3) * (nw - 1) for w, nw in zip(P.WAVELENGTHS, n)]
                np.testing.assert_allclose(block[9:11], scales, rtol=1e-14)
                np.testing.assert_allclose(block[11:] * scales[0], nodes.reshape(-1), rtol=1e-12)
                assert block.size == 11 + 24 * 18
            assert int(row["interaction"]) == (S.INTERACT_REFLECT if name == "radial_r"
                                               else S.INTERACT_REFRACT)
            if name == "tilted":
                assert int(row["flags"]) & S.SURF_ROTATED
            assert t.to_json() == P.case(name)["table"].to_json()   # the fixture's table, today
            # without the switch the surface is the reference's, as before
            plain = pack_surfaces(lens.surfaces.surfaces, [P.WAVELENGTH], tolerate=True)
            assert plain.phases == () and plain.unsupported == (G,)
            with pytest.raises(UnsupportedSystem):
                pack_surfaces(lens.surfaces.surfaces, [P.WAVELENGTH], phases=True)
            with pytest.raises(UnsupportedSystem):
                pack_optic(lens, [P.WAVELENGTH])
    finally:
        ref.set_backend("numpy")


@needs_reference
def test_packer_cache_is_shared_between_packs_with_and_without_phases(ref):
    from optiland_amd import fingerprint as fp
    from optiland_amd.packer import UnsupportedSystem, pack_surfaces

    lens = P.case_lens("radial_t")
    cache: dict = {}
    tok, keep = fp.surfaces_token(lens.surfaces.surfaces, P.WAVELENGTH)
    kw = dict(tokens=tok[1], cache=cache, keep=keep)
    t = pack_surfaces(lens.surfaces.surfaces, [P.WAVELENGTH], tolerate=True, phases=True, **kw)
    assert t.phases == (G,)
    plain = pack_surfaces(lens.surfaces.surfaces, [P.WAVELENGTH], tolerate=True, **kw)
    assert plain.phases == () and plain.unsupported == (G,)
    with pytest.raises(UnsupportedSystem):
        pack_surfaces(lens.surfaces.surfaces, [P.WAVELENGTH], **kw)
    again = pack_surfaces(lens.surfaces.surfaces, [P.WAVELENGTH], tolerate=True, phases=True, **kw)
    assert again.to_json() == t.to_json()
    both = pack_surfaces(lens.surfaces.surfaces, [P.WAVELENGTH], tolerate=True, phases=True,
                         gratings=True, **kw)
    assert both.to_json() == t.to_json()


@needs_reference
def test_packer_leaves_these_to_the_reference(ref):
    """A profile subclass, a BSDF, a Jones coating, an inhomogeneous medium, a degenerate grid, a
    height profile whose material has no n(), parameters that are not finite, a phase model on a
    curved geometry: each stays in `table.unsupported`."""
    from optiland.coatings import FresnelCoating
    from optiland.phase.radial import RadialPhaseProfile

    def left(lens):
        t = P.packed(lens)   # (a medium is shared with the next surface: that one may go too)
        return t.phases == () and G in t.unsupported

    def model(lens):
        return lens.surfaces.surfaces[G].interaction_model

    assert not left(P.lens("radial"))

    class Mine(RadialPhaseProfile):
        phase_type = "mine"

    lens = P.lens("radial")
    model(lens).phase_profile = Mine(list(P.RADIAL))
    assert left(lens)
    lens = P.lens("radial")
    model(lens).bsdf = object()
    assert left(lens)
    lens = P.lens("radial", material="N-BK7")
    surf = lens.surfaces.surfaces[G]
    model(lens).coating = FresnelCoating(surf.material_pre, surf.material_post)
    assert left(lens)
    lens = P.lens("radial")

    class Grin:
        pass

    Grin.__name__ = "GrinPropagation"
    surf = lens.surfaces.surfaces[G]
    was = surf.material_post.propagation_model
    surf.material_post.propagation_model = Grin()
    try:
        assert left(lens)
    finally:
        surf.material_post.propagation_model = was
    for bad in (float("nan"), float("inf")):
        assert left(P.lens("radial", coefficients=[-114.0, bad]))
        assert left(P.lens("constant", phase=bad))
    lens = P.lens("linear")
    model(lens).phase_profile._K_y = float("nan")
    assert left(lens)
    lens = P.lens("linear")
    model(lens).phase_profile._efficiency = float("inf")
    assert left(lens)
    # the phase model on a curved geometry is the reference's surface
    lens = P.lens("radial")
    from optiland.geometries.standard import StandardGeometry

    lens.surfaces.surfaces[G].geometry = StandardGeometry(lens.surfaces.surfaces[G].geometry.cs,
                                                          radius=80.0, conic=0.0)
    assert left(lens)
    _torch64(ref)
    try:
        for kind in ("grid", "height"):
            assert not left(P.lens(kind))
            lens = P.lens(kind)
            prof = model(lens).phase_profile
            prof.x_coords = prof.x_coords[:1]                  # fewer than 2 nodes on an axis
            assert left(lens)
            lens = P.lens(kind)
            prof = model(lens).phase_profile
            prof.y_coords = ref.array(np.full(18, 0.5))        # coincident end points
            assert left(lens)
            lens = P.lens(kind)
            prof = model(lens).phase_profile
            nodes = prof.phase_grid if kind == "grid" else prof.height_map
            nodes[3, 4] = float("nan")
            assert left(lens)
        lens = P.lens("height")
        model(lens).phase_profile.material = "N-BK7"           # a name: no n()
        assert left(lens)
    finally:
        ref.set_backend("numpy")


@needs_reference
@pytest.mark.parametrize("native", [True, False])
def test_surface_token_sees_every_phase_edit(ref, native):
    from optiland.materials import IdealMaterial
    from optiland_amd import fingerprint as fp

    if native and fp._NATIVE is None:
        # the native walk is an optional accelerator of the package, but it is the project's own
        # module: build it here rather than skip (a failure to build it fails the test)
        from optiland_amd import build

        build.build_fptoken(force=False, verbose=False)
        fp._NATIVE = fp._load_native()
        assert fp._NATIVE is not None, "csrc/fptoken.c built but does not load"
    assert fp.use_native(native) is native

    def token(lens):
        tok, _keep = fp.surfaces_token(lens.surfaces.surfaces, P.WAVELENGTH)
        return tok[1][G]

    def item(p):
        p.coefficients[1] = 0.5

    def node(p):
        a = p.phase_grid if hasattr(p, "phase_grid") else p.height_map
        a[2, 3] += 1.0

    def coord(p):
        p.x_coords[0] -= 0.01

    def index(p):
        p.material.index = p.material.index + 0.1

    edits = {
        "radial": [("an item of the list", item),
                   ("the list grows", lambda p: p.coefficients.append(1e-6)),
                   ("the list reassigned", lambda p: setattr(p, "coefficients", [-100.0]))],
        "linear": [("period", lambda p: setattr(p, "period", 4.0e-3)),
                   ("angle", lambda p: setattr(p, "angle", 0.3)),
                   ("order", lambda p: setattr(p, "order", 2)),
                   ("efficiency", lambda p: setattr(p, "_efficiency", 0.5)),
                   ("K_x", lambda p: setattr(p, "_K_x", 7.0))],
        "constant": [("phase", lambda p: setattr(p, "phase", 0.2))],
        "grid": [("a node in place", node), ("a coordinate in place", coord),
                 ("nodes reassigned", lambda p: setattr(p, "phase_grid", p.phase_grid.clone()
                                                         if hasattr(p.phase_grid, "clone")
                                                         else p.phase_grid.copy())),
                 ("y reassigned", lambda p: setattr(p, "y_coords", p.y_coords * 1.0))],
        "height": [("a node in place", node), ("a coordinate in place", coord),
                   ("material swapped", lambda p: setattr(p, "material", IdealMaterial(n=1.7))),
                   ("material edited in place", index)],
    }
    try:
        for backend in ("numpy", "torch"):
            if backend == "torch":
                _torch64(ref)
            else:
                ref.set_backend("numpy")
            for kind, todo in edits.items():
                if backend == "numpy" and kind in ("grid", "height"):
                    continue    # (built on the torch backend: the NumPy one needs SciPy's spline)
                for what, edit in todo:
                    lens = P.lens(kind)
                    prof = lens.surfaces.surfaces[G].interaction_model.phase_profile
                    if what == "material edited in place":
                        prof.material = IdealMaterial(n=1.5)
                    before = token(lens)
                    assert before == token(lens), what
                    edit(prof)
                    assert before != token(lens), (backend, kind, what)
    finally:
        fp.use_native(fp._NATIVE is not None)
        ref.set_backend("numpy")


# ------------------------------------------------------------------ the drop-in, end to end on CPU
@pytest.fixture()
def phase_on_cpu(ref, monkeypatch, hostphase, tmp_path):
    import optiland_amd.tracer as tr
    from optiland_amd import integration as I

    cls = P.make_engine_class(hostphase, tmp_path)
    cls.phase_launches = 0

    def factory(table, device):
        return cls(table, device)

    factory.traces_phases = True    # what the product's own factory declares
    monkeypatch.setattr(tr, "_make_engine", factory)
    monkeypatch.setitem(I._SG, "phases", True)
    be = ref
    _torch64(be)
    yield be, cls
    be.set_backend("numpy")


def _recorded(be, lens):
    return np.stack([np.stack([np.asarray(be.to_numpy(getattr(s, k)), dtype=np.float64).reshape(-1)
                               for k in ("x", "y", "z", "L", "M", "N", "intensity", "opd")])
                     for s in lens.surfaces.surfaces])


def _trace(be, lens, name):
    """The rays of the fixture's case -- row 0 of it -- through `lens.surfaces.trace`."""
    from optiland.rays import RealRays

    c = P.case(name)
    start = c["rows"][0]
    w = float(c["table"].wavelengths[c["wl"]])
    rays = RealRays(*[be.array(start[k].copy()) for k in range(7)], w)
    rays.opd = be.array(start[7].copy())
    lens.surfaces.trace(rays)
    return rays


@needs_reference
@pytest.mark.parametrize("name", ["radial_t", "radial_r", "linear_m1", "constant", "grid",
                                  "height_blue", "tir_p1"])
def test_dropin_traces_the_phase_plane_on_the_engine(phase_on_cpu, name):
    (be, cls) = phase_on_cpu
    from optiland_amd import integration as I

    c = P.case(name)
    g = c["g"]
    lens = P.case_lens(name)
    I.install(lens, force=True)
    foreign, served = I._SG["foreign"], I._SG["count"]
    rays = _trace(be, lens, name)
    assert I._SG["count"] == served + 1          # the group's trace was the bridge's
    assert I._SG["foreign"] == foreign           # and no surface went to the reference's own trace
    assert cls.phase_launches == 1
    got = _recorded(be, lens)
    upto = g + 1 if name in P.TIR_CASES else got.shape[0]    # (behind it N = 0: -z / N)
    scale = P.scale_of(c["rows"][:upto])
    assert got.shape == c["rows"].shape and not np.isnan(got[:upto]).any()
    P.compare(got[:upto], c["rows"][:upto], np.float64, scale, name, tight=True, report=print)
    np.testing.assert_array_equal(np.asarray(be.to_numpy(rays.L)), got[-1, 3])
    if name != "radial_t":
        return
    # an edit of a coefficient in place between two traces shows, as the reference's does
    prof = lens.surfaces.surfaces[g].interaction_model.phase_profile
    prof.coefficients[0] = -90.0
    _trace(be, lens, name)
    after = _recorded(be, lens)
    assert np.abs(after[g, 3:6] - got[g, 3:6]).max() > 1e-3
    I._SG["phases"] = False
    fresh = P.case_lens(name)
    fresh.surfaces.surfaces[g].interaction_model.phase_profile.coefficients[0] = -90.0
    I.install(fresh, force=True)
    _trace(be, fresh, name)
    P.compare(after, _recorded(be, fresh), np.float64, scale, name + " a_2 = -90", tight=True,
              report=print)
    assert cls.phase_launches == 2


@needs_reference
def test_dropin_polarised_bundle_takes_the_references_surface(phase_on_cpu):
    (be, cls) = phase_on_cpu
    from optiland.rays import PolarizationState
    from optiland_amd import integration as I

    lens = P.case_lens("radial_t")
    lens.updater.set_polarization(PolarizationState(is_polarized=False))
    I.install(lens, force=True)
    foreign = I._SG["foreign"]
    lens.trace(0.0, 1.0, P.WAVELENGTH, 6, "hexapolar")
    assert cls.phase_launches == 0 and I._SG["foreign"] == foreign + 1
    c = P.case("radial_t")
    got = _recorded(be, lens)
    np.testing.assert_allclose(got[:, :6], c["rows"][:, :6], rtol=0,
                               atol=1e-12 * P.scale_of(c["rows"]))


@needs_reference
def test_dropin_switch_and_subclass_send_the_plane_back_to_the_reference(phase_on_cpu):
    (be, cls) = phase_on_cpu
    from optiland.phase.radial import RadialPhaseProfile
    from optiland_amd import integration as I

    I._SG["phases"] = False      # what enable(phases=False) / OPTILAND_HIP_PHASES=0 set
    lens = P.case_lens("radial_t")
    I.install(lens, force=True)
    foreign = I._SG["foreign"]
    _trace(be, lens, "radial_t")
    assert cls.phase_launches == 0 and I._SG["foreign"] == foreign + 1
    c = P.case("radial_t")
    np.testing.assert_allclose(_recorded(be, lens), c["rows"], rtol=0,
                               atol=1e-12 * P.scale_of(c["rows"]))
    # and back on: the same lens, the next trace
    I._SG["phases"] = True
    _trace(be, lens, "radial_t")
    assert cls.phase_launches == 1 and I._SG["foreign"] == foreign + 1

    class Mine(RadialPhaseProfile):
        phase_type = "mine_too"

    lens.surfaces.surfaces[G].interaction_model.phase_profile = Mine(list(P.RADIAL))
    _trace(be, lens, "radial_t")
    assert cls.phase_launches == 1 and I._SG["foreign"] == foreign + 2
    np.testing.assert_allclose(_recorded(be, lens), c["rows"], rtol=0,
                               atol=1e-12 * P.scale_of(c["rows"]))


@needs_reference
def test_a_factory_that_declares_nothing_gets_todays_table(ref, monkeypatch):
    """The seam decides before packing: an engine factory without `traces_phases` (every stand-in
    of the existing suite) never sees a phase row."""
    import optiland_amd.tracer as tr
    from optiland_amd import integration as I

    assert getattr(tr._make_engine, "traces_phases", False) is True
    monkeypatch.setitem(I._SG, "phases", True)
    lens = P.case_lens("radial_t")
    t = I._sg_table(lens.surfaces, P.WAVELENGTH)
    assert t.phases == (G,) and t.unsupported == ()
    monkeypatch.setattr(tr, "_make_engine", lambda table, device: None)
    t = I._sg_table(lens.surfaces, P.WAVELENGTH)
    assert t.phases == () and t.unsupported == (G,)


@needs_reference
def test_enable_takes_the_switch(ref):
    from optiland_amd import integration as I

    was = I._SG["phases"]
    try:
        I.enable(force=True, analyses=False, phases=False)
        assert I._SG["phases"] is False
        I.enable(force=True, analyses=False)
        assert I._SG["phases"] is False     # None leaves it as it is
        I.enable(force=True, analyses=False, phases=True)
        assert I._SG["phases"] is True
    finally:
        I.disable()
        I._SG["phases"] = was
