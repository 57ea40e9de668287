#!/usr/bin/env python
"""tests/golden/grid_sag.npz: the reference's grid-sag surfaces (geometries/grid_sag.py, surface
type "grid_sag") traced by its own `SurfaceGroup.trace` on the NumPy backend in fp64, for
tests/test_grid_sag_cpu.py and tests/test_gpu_grid_sag.py.  Optics, grids, fields and ray sets are
tests/_grid_sag.py's (`CASES`): a singlet whose front surface is a sampled sphere plus a smooth
ripple.  Each case is traced at one field (0 or 1, alternating over the cases) and three small
cases with 127 rays instead of 469: both fields of every case at both tolerances do not fit the
size limit of a committed file.  Per case:

  table                  the packed table (JSON text, `pack_surfaces(tolerate=True, grid_sags=True)`)
  before (8, n)          the rays in front of the grid-sag surface, x y z L M N intensity opd
  tight/after, tight/lens        (8, n) the surface's recorded row and the image surface's, the
  factory/after, factory/lens    geometry's tol at 1e-12 and at the factory's 1e-6
  residual (2,)          the largest |sag(x, y) - z| at the reference's hits, tight and factory
  nan (2,)               how many rays left the grid
and `known_*`: the known answers of the reference's tests/test_grid_sag_geometry.py as data -- the
ray at (0, 0, -1) along +z onto the plane sag = 0.1 x travels 1.0 and finds the normal
(-0.1, 0, 1) / |.|.

Asserted here: at the reference's returned hit |sag(x, y) - z| <= 1e-13 for EVERY ray that is not
NaN, at both tolerances (no ray is excluded for non-convergence; a case that fails is changed, not
the bound); every hit exactly on a grid line or at least 2e-5 mm from the nearest (the slope jumps
there: tests/_grid_sag.py); NaN rays only in the narrow case, and there between 2 and 50 % of the bundle; clipped
rays in the clipped case; the rays of the nodes case ON node coordinates; the known answers.

    python tools/make_golden_grid_sag.py        (needs the reference package; CPU only)
"""

from __future__ import annotations

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

from tests import _grid_sag as G  # noqa: E402

PLANES = ("x", "y", "z", "L", "M", "N", "intensity", "opd")


def _np(v):
    return np.asarray(be.to_numpy(v), dtype=np.float64).reshape(-1)


def recorded(optic, n):
    return np.stack([np.stack([np.broadcast_to(_np(getattr(s, k)), (n,)).copy() for k in PLANES])
                     for s in optic.surfaces.surfaces])


def trace_rows(optic, hx, hy, px, py):
    """(S + 1, 8, n): what every surface recorded of one `SurfaceGroup.trace`."""
    n = px.size
    rays = optic.ray_tracer.ray_generator.generate_rays(
        be.array(np.full(n, hx)), be.array(np.full(n, hy)), be.array(px), be.array(py),
        G.WAVELENGTH)
    with np.errstate(invalid="ignore"):
        optic.surfaces.trace(rays)
    return recorded(optic, n)


def known_answers(out):
    from optiland.rays import RealRays

    optic = G.lens(1e-6, plane=True, epd=1.6)
    table = G.packed(optic)
    surf = optic.surfaces.surfaces[G.GRID]
    z0 = float(_np(surf.geometry.cs.z)[0])
    before = np.array([0.0, 0.0, z0 - 1.0, 0.0, 0.0, 1.0, 1.0, 0.0])
    rays = RealRays(*[be.array([v]) for v in before[:7]], G.WAVELENGTH)
    surf.trace(rays)
    after = np.array([_np(getattr(surf, k))[0] for k in PLANES])
    np.testing.assert_allclose(after[:3], [0.0, 0.0, z0], rtol=0, atol=1e-5)   # distance 1.0
    np.testing.assert_allclose(after[7], 1.0, rtol=0, atol=1e-5)
    n1, n2 = float(table.optics["n1"][G.GRID, 0]), float(table.optics["n2"][G.GRID, 0])
    nrm = np.array([-0.1, 0.0, 1.0]) / np.sqrt(1.01)
    k0 = np.array([0.0, 0.0, 1.0])
    u, dot = n1 / n2, float(nrm @ k0)
    want = u * k0 + nrm * (np.sqrt(1 - u * u * (1 - dot * dot)) - u * dot)
    np.testing.assert_allclose(after[3:6], want, rtol=0, atol=1e-5)
    out["known_table"] = np.array(table.to_json())
    out["known_in"], out["known_out"], out["known_direction"] = before, after, want


def main():
    be.set_backend("numpy")
    out, names = {}, []
    for name, (_edit, (hx, hy), rayset) in G.CASES.items():
        px, py = G.pupil_points(rayset)
        rows = {}
        for key, tol in G.TOLS.items():
            optic = G.case_lens(name, tol)
            table = G.packed(optic)
            assert table.grid_sag_rows == (G.GRID,) and table.unsupported == (), \
                (name, table.unsupported)
            assert float(table.surfaces["tol"][G.GRID]) == tol
            rows[key] = trace_rows(optic, hx, hy, px, py)
        g = G.GRID
        assert np.array_equal(rows["tight"][g - 1], rows["factory"][g - 1])
        before = rows["tight"][g - 1]
        assert not np.isnan(before).any(), name
        res, nans = [], []
        for key in G.TOLS:
            after = rows[key][g]
            lost = np.isnan(after[0])
            # a ray is NaN in all of position and direction or in none of them
            assert np.array_equal(np.isnan(after[:6]).all(axis=0), lost), name
            assert np.array_equal(np.isnan(after[:6]).any(axis=0), lost), name
            r = G.residual(table, g, after)
            assert np.array_equal(np.isnan(r), lost), name
            worst = float(np.nanmax(r))
            assert worst <= G.RESIDUAL, (name, key, worst)
            res.append(worst)
            d = G.grid_line_distance(table, g, after)[:, ~lost]
            assert ((d == 0.0) | (d >= G.LINE_MARGIN)).all(), (name, key, float(d[d > 0].min()))
            nans.append(int(lost.sum()))
            if name in G.NAN_CASES:
                assert 0.02 <= lost.mean() <= 0.5, (name, key, float(lost.mean()))
            else:
                assert not lost.any(), (name, key, int(lost.sum()))
        assert nans[0] == nans[1], (name, nans)
        if name == "clipped":
            hit = rows["tight"][g, 6] == 0.0
            assert hit.any() and not hit.all(), "the aperture clips nothing / everything"
        if name == "nodes":
            xs, ys, _z = G.block_of(table, g)
            p = G.local_point(table, g, rows["tight"][g])
            on_x, on_y = np.isin(p[0], xs), np.isin(p[1], ys)
            assert (on_x & on_y).sum() >= 40 and (on_x ^ on_y).sum() >= 20, \
                (int((on_x & on_y).sum()), int((on_x ^ on_y).sum()))
            assert (p[0] == 0.0).any() and (p[1] == 0.0).any()
        print(f"{name}: {before.shape[1]} rays, NaN {nans[0]}, residual tight {res[0]:.3g} "
              f"factory {res[1]:.3g}", flush=True)
        names.append(name)
        table.surfaces["tol"][g] = G.TOLS["tight"]   # (`case` sets the one it is asked for)
        out[f"{name}/table"] = np.array(table.to_json())
        out[f"{name}/before"] = before
        for key in G.TOLS:
            out[f"{name}/{key}/after"] = rows[key][g]
            out[f"{name}/{key}/lens"] = rows[key][-1]
        out[f"{name}/residual"] = np.array(res)
        out[f"{name}/nan"] = np.array(nans)
    known_answers(out)
    out["cases"] = np.array(names)
    np.savez_compressed(G.GOLD, **out)
    size = os.path.getsize(G.GOLD)
    print(f"{G.GOLD}: {size} bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
