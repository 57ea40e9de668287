"""The ensemble wavefront trace (`ol_trace_opd_ensemble`) without a GPU: the declaration and the
cell record's layout, `opd_cell_grid`, the cells of csrc/ensemble_opd_device.h run on the CPU by
the stand-alone program tests/hostensemble_opd -- against the reference fixture
tests/golden/ensemble_opd.npz (tests/_ensemble_opd.py) under the bounds tests/test_wavefront.py
holds `ol_trace_opd` to, plain and under the sanitizers -- and `tolerancing.monte_carlo`'s replay
and refusals.  No GPU needed."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from optiland_amd import _capi
from tests import _ensemble as E
from tests import _ensemble_opd as EO
from tests import _live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = pytest.mark.skipif(not EO._builder().available(), reason="needs hipcc (host compile)")
needs_reference = pytest.mark.skipif(_live.reference_root() is None,
                                     reason="needs the reference package")


# ------------------------------------------------------------------ declaration, layout
def test_the_entry_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "optiland_hip.h")).read()
    assert "int ol_trace_opd_ensemble(const ol_ensemble* ens, ol_dtype dt, int64_t n_rays," in text
    assert "#define OL_OPD_ENSEMBLE_PUPIL 0x100u" in text
    assert "#define OL_ABI_VERSION 11" in text
    assert "ol_trace_opd_ensemble" in _capi.EXPORTS and _capi.ABI_VERSION == 11
    assert _capi.OPD_ENSEMBLE_PUPIL == 0x100


def test_the_cell_record_has_one_layout():
    """numpy dtype == ctypes Structure == what gcc lays out for the header."""
    from optiland_amd.ensemble import OPD_CELL_DTYPE
    names = [n for n, _t in _capi.EnsembleOpdCell._fields_]
    assert list(OPD_CELL_DTYPE.names) == names
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"optiland_hip.h\"\n" \
        + "int main(void) {\n" \
        + "".join(f'  printf("%zu ", offsetof(ol_ensemble_opd_cell, {n}));\n' for n in names) \
        + '  printf("%zu\\n", sizeof(ol_ensemble_opd_cell));\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        nums = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert nums[-1] == OPD_CELL_DTYPE.itemsize == C.sizeof(_capi.EnsembleOpdCell)
    for off, n in zip(nums, names):
        assert off == OPD_CELL_DTYPE.fields[n][1] == getattr(_capi.EnsembleOpdCell, n).offset, n


def test_cells_are_filled_from_their_own_variant():
    from optiland_amd.ensemble import opd_cell_grid
    for lens in E.LENSES:
        tabs, a = EO.tables(lens), EO.arrays(lens)
        wl = EO.wavelength_indices(lens, tabs[0])
        cells = opd_cell_grid(tabs, a["fields"], wl, planar=False)
        K, F, W = len(tabs), len(a["fields"]), len(wl)
        assert cells.shape == (K, F, W)
        for k, t in enumerate(tabs):
            c = cells[k]
            assert (c["variant"] == k).all()
            assert (c["n_image"] == t.raygen["n_image"]).all()
            assert (c["pupil_z"] == t.raygen["pupil_z"]).all()
            assert (c["last_thickness"] == t.last_thickness).all() and (c["planar"] == 0).all()
            assert (c["wavelength_um"] == a["wavelengths"][None, :]).all()
            assert (c["wavelength_index"] == np.asarray(wl)[None, :]).all()
            assert (c["hx"] == a["fields"][:, 0, None]).all()
            assert (c["hy"] == a["fields"][:, 1, None]).all()
            assert (c["vx"] == 1).all() and (c["vy"] == 1).all()
        # The radius in front of the stop moves the ENTRANCE pupil (the variant's own ray-
        # generation constants, on the device); both lenses state an entrance-pupil diameter and
        # their exit pupil is formed behind the stop, so what the CELL carries moves with the
        # thickness variant: its image plane, hence its exit-pupil position, is its own
        assert tabs[E.RADIUS_VARIANT].raygen["EPL"] != tabs[0].raygen["EPL"]
        moved = cells["pupil_z"][EO.THICKNESS_VARIANT, 0, 0]
        assert moved != cells["pupil_z"][0, 0, 0] and \
            moved == tabs[EO.THICKNESS_VARIANT].raygen["pupil_z"]
    assert (opd_cell_grid(tabs[:1], [(0, 0)], [0], planar=True)["planar"] == 1).all()
    bare = EO.tables("cooke")[:1]
    del bare[0].raygen["pupil_z"]
    with pytest.raises(ValueError, match="carries no exit-pupil data"):
        opd_cell_grid(bare, [(0, 0)], [0])


# ------------------------------------------------------------------ the host program
@host
@pytest.mark.parametrize("lens", E.LENSES)
def test_host_walk_holds_the_fixture(lens):
    a = EO.arrays(lens)
    K, F, W, N = a["opd"].shape
    got = EO.host_walk(lens)
    assert got["status"] == 0
    rays = got["rays"].reshape(K, F, W, 5, N)
    checks = EO.opd_checks(lens, rays[..., 0, :], rays[..., 1, :], a["opd"], a["intensity"])
    radius = got["refs"][:, 3].reshape(K, F, W)
    checks.append((f"{lens} radius (relative)",
                   float(np.abs(radius / a["radius"] - 1.0).max()), EO.RADIUS_RTOL))
    # the moments the program sums are those of its own map
    lit = rays[..., 1, :] > 0
    mom = got["mom"].reshape(K, F, W, 12)
    checks.append((f"{lens} count", float(np.abs(mom[..., 9] - lit.sum(-1)).max()), 0.0))
    if lens == "cooke":
        kept = lit.sum(-1)
        assert kept[E.CLIPPED_VARIANT, 1, 0] == EO.CLIPPED_KEPT and (kept[0] == N).all()
    EO.report(checks)


@host
@pytest.mark.parametrize("lens", E.LENSES)
def test_host_walk_holds_the_operand(lens):
    """`RayOperand.OPD_difference` formed from the program's maps at the operand's own quadrature
    points, under the bounds of the maps."""
    a = EO.arrays(lens)
    K, F, W = a["operand"].shape
    got = np.zeros((K, F, W))
    for f in range(F):
        on_axis = bool((a["fields"][f] == 0).all())
        which = "gq_axis" if on_axis else "gq_field"
        _px, _py, weights = EO.quadrature(on_axis)
        rays = EO.host_walk(lens, which)["rays"].reshape(K, F, W, 5, weights.size)
        for k in range(K):
            for w in range(W):
                got[k, f, w] = EO.operand_from_opd(rays[k, f, w, 0], weights)
    scale = max(1.0, float(np.abs(a["opd"][a["intensity"] > 0]).max()))
    EO.report([(f"{lens} OPD_difference [waves]", float(np.abs(got - a["operand"]).max()),
                EO.OPD_BOUND[lens] * scale)])


@host
def test_host_walk_under_the_sanitizers(tmp_path):
    """The stand-alone program with AddressSanitizer + UndefinedBehaviorSanitizer linked in: the
    stacked tables, the variant strides, the chief ray and the cell walk read nothing they do not
    own -- also for cells that name a variant or a wavelength row outside the ensemble, which are
    skipped."""
    tabs, a = EO.tables("singlet"), EO.arrays("singlet")
    cells = EO.cells("singlet", tabs).reshape(-1).copy()
    cells["variant"][3] = len(tabs)
    cells["variant"][4] = -1
    cells["wavelength_index"][5] = 2
    path = os.path.join(str(tmp_path), "case.bin")
    EO.write_case(path, tabs, a["px"], a["py"], cells)
    plain, rc, err = EO.run_host(path)
    assert rc == 0 and not err, err
    checked, rc, err = EO.run_host(path, sanitize=True)
    assert rc == 0 and not err, err
    assert checked == plain
    got = EO.parse(plain, cells.size, a["px"].size)
    assert got["status"] == _capi.STATUS_ENSEMBLE_CELL and not got["errors"]
    assert np.isnan(got["rays"][3:6]).all() and np.isnan(got["refs"][3:6]).all()
    assert not np.isnan(got["rays"][:3, 0]).any() and not np.isnan(got["refs"][:3]).any()


# ------------------------------------------------------------------ the bridge
class _FakeSystem:
    """Stand-in for `engine.HipSystem` in tests/_fake_engine.py's style (the oracle behind the
    calls the per-variant loop makes): `update`, `wavefront_reference`, `trace_opd(reference=)`."""

    made = []

    def __init__(self, table, device=None):
        from tests._fake_engine import OracleEngine
        self.oracle = OracleEngine(table, "cpu")
        self.device = self.oracle.device
        self.log = []
        _FakeSystem.made.append(self)

    def update(self, table):
        self.oracle.table = table
        self.log.append("update")
        return True

    def close(self):
        self.log.append("close")

    def wavefront_reference(self, params, wl_index, *, field, vig=(1.0, 1.0), pupil_z=0.0,
                            planar=False, want_chief=False, zero_status=True):
        import torch
        zero = torch.zeros(1, dtype=torch.float64)
        rays = self.oracle.generate_rays(float(field[0]), float(field[1]), zero, zero,
                                         float(vig[0]), float(vig[1])) \
            + [torch.zeros(1, dtype=torch.float64)]
        self.oracle.trace(rays, wl_index, record=False)
        x, y, z, L, M, N, _i, opd = (float(r[0]) for r in rays)
        R = math.sqrt(x * x + y * y + (z - pupil_z) ** 2)
        a = L * L + M * M + N * N
        t_back = math.sqrt(4.0 * a * R * R) / (2.0 * a)
        self.log.append(("reference", tuple(field), int(wl_index)))
        return dict(params, xc=x, yc=y, zc=z, R=R, opd_ref=opd - params["n_image"] * t_back), None

    def trace_opd(self, params, px, py, wl_index, *, field, want_pupil=True, reference=None,
                  zero_status=True, **_kw):
        assert params is None and reference is not None
        self.log.append(("opd", tuple(field), int(wl_index), int(px.numel())))
        return self.oracle.trace_opd(reference, px, py, wl_index, field=field,
                                     want_pupil=want_pupil)


def _problem(seed=11):
    tol = EO.tolerancing_problem(seed)
    tol.operands = tol.operands[:2]      # the two OPD_difference operands
    return tol


@pytest.mark.reference
@needs_reference
def test_monte_carlo_replays_the_reference_loop(monkeypatch):
    _live.import_reference()
    from optiland.tolerancing.monte_carlo import MonteCarlo

    from optiland_amd import engine
    from optiland_amd.tolerancing import monte_carlo
    iterations = 4
    ref = _problem()
    mc = MonteCarlo(ref)
    mc.run(iterations)
    want = mc.get_results() if hasattr(mc, "get_results") else mc._results
    _FakeSystem.made = []
    monkeypatch.setattr(engine, "HipSystem", _FakeSystem)
    got = monte_carlo(_problem(), iterations, "cpu")       # (below the minimum: the loop)
    pert, names = [str(p.variable) for p in ref.perturbations], mc.operand_names
    assert len(got) == iterations and list(got[0]) == pert + names
    for k in range(iterations):
        for key in pert:
            assert got[k][key] == float(want[key][k]), (k, key)      # the reference's own draws
    # ONE system, re-written per variant; per variant each operand's two launches, the on-axis
    # operand on the symmetric quadrature (3 points), the other on 9
    (fake,) = _FakeSystem.made
    per_variant = [("reference", (0.0, 0.0), 0), ("opd", (0.0, 0.0), 0, 3),
                   ("reference", (0.0, 0.7), 0), ("opd", (0.0, 0.7), 0, 9)]
    assert fake.log == per_variant + (["update"] + per_variant) * (iterations - 1) + ["close"]
    # the oracle restates the reference: its operands are the reference's to the kernels' bound
    worst = max(abs(got[k][n] - float(want[n][k])) for k in range(iterations) for n in names)
    print(f"OPD_difference, oracle loop against the reference: {worst:.3e} waves")
    assert worst <= EO.OPD_BOUND["cooke"]


@pytest.mark.reference
@needs_reference
def test_what_monte_carlo_does_not_serve_is_refused_before_anything_moves():
    from optiland_amd.packer import UnsupportedSystem, pack_optic
    from optiland_amd.tolerancing import monte_carlo
    wls = [0.48, 0.55]
    tol = EO.tolerancing_problem()
    before = pack_optic(tol.optic, wls)
    tol.add_compensator("thickness", surface_number=6)
    with pytest.raises(UnsupportedSystem, match="compensators"):
        monte_carlo(tol, 4, "cpu")
    tol = EO.tolerancing_problem()
    tol.add_operand("seidel", dict(optic=tol.optic, seidel_number=1))
    with pytest.raises(UnsupportedSystem, match="operand 3 is 'seidel'"):
        monte_carlo(tol, 4, "cpu")
    tol = EO.tolerancing_problem()
    # (the reference's OPD_difference cannot take "all" itself; its rms_spot_size can)
    tol.add_operand("rms_spot_size", dict(optic=tol.optic, surface_number=-1, Hx=0.0, Hy=0.0,
                                          num_rays=5, wavelength="all", distribution="hexapolar"))
    with pytest.raises(UnsupportedSystem, match="wavelength='all'"):
        monte_carlo(tol, 4, "cpu")
    assert all(p.value is None for p in tol.perturbations)          # nothing was drawn
    assert pack_optic(tol.optic, wls).surfaces.tobytes() == before.surfaces.tobytes()
