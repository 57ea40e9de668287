#!/usr/bin/env python
"""tests/golden/phase.npz: the reference's phase surfaces (a Plane with
interactions/phase_interaction_model.py and the profiles of optiland/phase/) traced by its own
`SurfaceGroup.trace` on the CPU in fp64, for tests/test_phase_cpu.py and tests/test_gpu_phase.py.
Optics, variants, fields and ray sets are tests/_phase.py's (`CASES`).  The analytic profiles are
traced on the NumPy backend; the gridded ones (`TORCH_CASES`) on the torch backend with
set_precision("float64"): its bilinear grid_sample is what the device reproduces, the NumPy
backend's spline is another interpolant.  Per case:

  table                  the packed table (JSON text, `pack_surfaces(tolerate=True, phases=True)`)
  g, wl                  index of the phase row, wavelength index of the trace
  rows (S + 1, 8, n)     every recorded row of the 127-ray hexapolar set, x y z L M N intensity opd
                         (row 0 is the object surface's: the input rays)
  dropped (2,)           how many of the 127 rays went at the radicand and at grid lines
  big_in, big_out (8, m) BIG_CASES only: rows g - 1 and g of the 1027-ray set
and `known_*`: the known answers of the reference's tests/test_phase_interaction_model.py and
tests/test_radial_phase.py as data -- `known_table` (JSON per entry), `known_in` / `known_out`
(the ray in front of the plane and what the reference's Surface.trace made of it) and
`known_want` (the constant of that file the entry is checked against, see `KNOWN`).

Rays with |S| / n2'^2 < 1e-2 and rays within 1e-4 of a cell pitch of a grid line are dropped
before saving.  Asserted here: both margins, 10-90 % clipped rays in the TIR cases and no
TIR-clipped ray elsewhere, at most 1 % of a case's rays gone at grid lines, clipped rays in the
clipped case, hits outside the grid (within one cell and further out) in the grid case, the known
answers.

    python tools/make_golden_phase.py        (needs the reference package; CPU only)
"""

from __future__ import annotations

import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# the reference package: OPTILAND_REFERENCE, else the copy build() staged under oracle/_ref
REF = os.environ.get("OPTILAND_REFERENCE") or os.path.join(ROOT, "oracle", "_ref")
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.join(ROOT, "tests", "refshim"), ROOT, REF]   # (ROOT first: `tests` is ours)

import numpy as np  # noqa: E402

import optiland.backend as be  # noqa: E402

from tests import _phase as P  # noqa: E402

PLANES = ("x", "y", "z", "L", "M", "N", "intensity", "opd")

# the reference's known answers: (what, radial coefficients, reflecting, wavelength, ray (x, y))
#   L        tests/test_phase_interaction_model.py: a metalens of f = 100 into n = 1.5 sends the
#            ray at x = 1 to L = -x / (n2 f), M = 0 (atol 1e-6)
#   N<0      ...: the same reflecting: N < 0
#   i=0      ...: coefficient 1e6: evanescent, intensity 0
#   phi      tests/test_radial_phase.py: [0.5, 0.1] at (1, 0), (2, 1), (0, 0): 0.6, 5.0, 0
#   grad     ...: [0.5] at (1, 0), (0, 2), (3, 4), (0, 0): the gradient is (x, y)
_K0 = 2 * math.pi / (0.5 * 1e-3)
KNOWN = (
    ("L", [-_K0 / 200.0], False, (1.0, 0.0), -1.0 / 150.0),
    ("N<0", [-_K0 / 200.0], True, (1.0, 0.0), 0.0),
    ("i=0", [1e6], False, (1.0, 0.0), 0.0),
    ("phi", [0.5, 0.1], False, (1.0, 0.0), 0.6),
    ("phi", [0.5, 0.1], False, (2.0, 1.0), 5.0),
    ("phi", [0.5, 0.1], False, (0.0, 0.0), 0.0),
    ("grad", [0.5], False, (1.0, 0.0), 0.0),
    ("grad", [0.5], False, (0.0, 2.0), 0.0),
    ("grad", [0.5], False, (3.0, 4.0), 0.0),
    ("grad", [0.5], False, (0.0, 0.0), 0.0),
)
KNOWN_WAVELENGTH = 0.5


def _np(v):
    return np.asarray(be.to_numpy(v), dtype=np.float64).reshape(-1)


def recorded(optic, n):
    return np.stack([np.stack([np.broadcast_to(_np(getattr(s, k)), (n,)).copy() for k in PLANES])
                     for s in optic.surfaces.surfaces])


def trace_rows(optic, hx, hy, px, py, wavelength):
    """(S + 1, 8, n): what every surface recorded of one `SurfaceGroup.trace`."""
    n = px.size
    rays = optic.ray_tracer.ray_generator.generate_rays(
        be.array(np.full(n, hx)), be.array(np.full(n, hy)), be.array(px), be.array(py),
        wavelength)
    with np.errstate(invalid="ignore"):
        optic.surfaces.trace(rays)
    return recorded(optic, n)


def use_backend(name):
    be.set_backend(name)
    if name == "torch":
        be.set_device("cpu")
        be.set_precision("float64")


def known_answers(out):
    from optiland.materials import IdealMaterial

    use_backend("numpy")
    tables, k_in, k_out, k_want, k_what = [], [], [], [], []
    for what, coeffs, reflect, (x, y), want in KNOWN:
        optic = P.lens("radial", coefficients=coeffs,
                       material="mirror" if reflect else IdealMaterial(n=1.5))
        table = P.packed(optic, [KNOWN_WAVELENGTH])
        assert table.phases == (P.PHASE,) and table.unsupported == ()
        surf = optic.surfaces.surfaces[P.PHASE]
        z = float(_np(surf.geometry.cs.z)[0])
        from optiland.rays import RealRays

        rays = RealRays(be.array([x]), be.array([y]), be.array([z]), be.array([0.0]),
                        be.array([0.0]), be.array([1.0]), be.array([1.0]), KNOWN_WAVELENGTH)
        before = np.array([x, y, z, 0.0, 0.0, 1.0, 1.0, 0.0])
        surf.trace(rays)
        after = np.array([_np(getattr(surf, k))[0] for k in PLANES])
        q = KNOWN_WAVELENGTH * 1e-3 / (2 * math.pi)
        if what == "L":
            np.testing.assert_allclose(after[3], want, rtol=0, atol=1e-6)
            np.testing.assert_allclose(after[4], 0.0, rtol=0, atol=1e-6)
        elif what == "N<0":
            assert after[5] < 0
        elif what == "i=0":
            assert after[6] == 0.0
        elif what == "phi":
            np.testing.assert_allclose(-after[7] / q, want, rtol=1e-7, atol=1e-9)
        else:   # n2' (L, M) / q is the gradient: (x, y)
            np.testing.assert_allclose(after[3:5] * 1.5 / q, [x, y], rtol=1e-7, atol=1e-9)
        tables.append(table.to_json())
        k_in.append(before)
        k_out.append(after)
        k_want.append(want)
        k_what.append(what)
    out["known_table"] = np.array(tables)
    out["known_in"], out["known_out"] = np.array(k_in), np.array(k_out)
    out["known_want"], out["known_what"] = np.array(k_want), np.array(k_what)


def main():
    out, names = {}, []
    for name, (_kind, _edit, (hx, hy), wl) in P.CASES.items():
        use_backend("torch" if name in P.TORCH_CASES else "numpy")
        optic = P.case_lens(name)
        wavelengths = P.case_wavelengths(name)
        table = P.packed(optic, wavelengths)
        g = P.PHASE
        assert table.phases == (g,) and table.unsupported == (), (name, table.unsupported)
        block = P.block_of(table, g)
        sets = {"hex127": trace_rows(optic, hx, hy, *P.pupil_points("hex127"), wavelengths[wl])}
        if name in P.BIG_CASES:
            sets[P.BIG_SET] = trace_rows(optic, hx, hy, *P.pupil_points(P.BIG_SET),
                                         wavelengths[wl])
        for key, rows in list(sets.items()):
            s = P.radicand(table, g, rows[g - 1], rows[g], wl)
            x, y = P.local_hit(table, g, rows[g])
            d = P.grid_line_distance(block, x, y)
            at_s, at_grid = np.abs(s) < P.MARGIN, d < P.GRID_MARGIN
            assert at_grid.mean() <= P.GRID_DROP_CAP, (name, key, float(at_grid.mean()))
            keep = ~(at_s | at_grid)
            rows = sets[key] = rows[:, :, keep]
            s = s[keep]
            # (behind the plane an evanescent ray has N = 0 exactly: the image plane's -z / N
            # makes it inf / NaN in the reference too)
            assert not np.isnan(rows[:g + 1]).any(), name
            assert name in P.TIR_CASES or not np.isnan(rows).any(), name
            # the reference clips exactly the rays with S < 0 -- on top of what the aperture took
            tir = s < 0
            assert np.all(rows[g, 6][tir] == 0.0), name
            if name in P.TIR_CASES:
                assert 0.1 <= tir.mean() <= 0.9, (name, float(tir.mean()))
                assert np.array_equal(rows[g, 6] == 0.0, tir), name
            else:
                assert not tir.any(), name
            if key == "hex127":
                out[f"{name}/dropped"] = np.array([int(at_s.sum()), int((at_grid & ~at_s).sum())])
            print(f"{name} {key}: kept {int(keep.sum())} of {keep.size} (radicand "
                  f"{int(at_s.sum())}, grid lines {int(at_grid.sum())}), TIR {tir.mean():.2f}, "
                  f"min |S|/n2'^2 {np.abs(s).min():.3g}", flush=True)
        rows = sets["hex127"]
        if name == "clipped":
            hit = rows[g, 6] == 0.0
            assert hit.any() and not hit.all(), "the aperture clips nothing / everything"
        if name == "grid":
            for key in sets:
                ix, iy = P.grid_coordinates(block, *P.local_hit(table, g, sets[key][g]))
                W, H = int(block[2]), int(block[3])
                far = np.maximum(np.maximum(-ix, ix - (W - 1)), np.maximum(-iy, iy - (H - 1)))
                assert ((far > 0) & (far < 1)).any() and (far > 1).any() and (far < 0).any(), \
                    "hits inside the grid, within one cell outside it and further out"
                print(f"grid {key}: {int(((far > 0) & (far < 1)).sum())} hits within one cell "
                      f"outside, {int((far >= 1).sum())} further out", flush=True)
        names.append(name)
        out[f"{name}/table"] = np.array(table.to_json())
        out[f"{name}/g"] = np.int64(g)
        out[f"{name}/wl"] = np.int64(wl)
        out[f"{name}/rows"] = rows
        if name in P.BIG_CASES:
            out[f"{name}/big_in"] = sets[P.BIG_SET][g - 1]
            out[f"{name}/big_out"] = sets[P.BIG_SET][g]
    known_answers(out)
    use_backend("numpy")
    out["cases"] = np.array(names)
    np.savez_compressed(P.GOLD, **out)
    size = os.path.getsize(P.GOLD)
    print(f"{P.GOLD}: {size} bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
