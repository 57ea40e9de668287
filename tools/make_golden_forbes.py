#!/usr/bin/env python
"""tests/golden/forbes.npz: the reference's Forbes surfaces (geometries/forbes/geometry.py,
qpoly.py; ForbesQNormalSlopeGeometry = "forbes_qbfs", ForbesQ2dGeometry = "forbes_q2d") traced
by its own `SurfaceGroup.trace` on the NumPy backend (CPU, fp64), for tests/test_forbes_cpu.py and
tests/test_gpu_forbes.py.  The lens, its variants and the ray sets are tests/_forbes.py's.

Cases `<kind>_<variant>_<tight|default>`: kind q / q2d; variant norm12 (all hits inside the
disc), norm8 (hits on both sides of u = 1), tilted (rx 0.03, dy 0.4), mirror, flat (infinite base
radius), clipped (RadialAperture r_max 7); solver tol 1e-12 ("tight") and the factory's 1e-6.
Ray sets, concatenated along the ray axis: the Hy = 1 hexapolar pupil of 6 rings (127 rays) and
the on-axis chief ray (1 ray) in every case; 1027 points uniform over the pupil at Hy = 0.5 in the
norm8 cases (the file must stay under 1 MB).  Per case:

  kind, variant, tol, table            the packed table (JSON text, `pack_surfaces(tolerate=True)`)
  set_names, set_lo, set_hi            the ray sets' slices of the ray axis
  rows (S + 1, 8, n)                   tight: every recorded row, x y z L M N intensity opd (row 0
                                       is the object surface's: the input rays)
  tight, delta (S + 1, 8, n) float32   default: the name of its tight case and rows - tight rows
                                       (they differ by <= 1e-10: float32 keeps that to 1e-17)
  spread (S + 1, 8)                    max |NumPy - torch| per array (the reference's torch
                                       backend, CPU, fp64), this tolerance
  gap (S + 1, 8)                       tight: max |tol 1e-12 - tol 1e-14| per array (NumPy)
and per geometry and base (`grid_<kind>_<norm12|flat>/`): x, y (33 x 33 over |x|, |y| <= 1.2
norm_radius, (0, 0) among them, plus points at u = 1 -+ 1e-9 and 1 -+ 2e-3 on both axes), sag,
normal (3, n) and their NumPy-to-torch spreads.

Asserted here: no NaN where none is expected (only clipped / missed rays may differ in
intensity), the NaN patterns of the backends agree, and at most 2 % of a Q2D case's rays hit
within |u - 1| < 1e-3 (the exclusion of the tests).

    python tools/make_golden_forbes.py        (needs the reference package; CPU only, ~1 min)
"""

from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("OPTILAND_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.join(ROOT, "tests", "refshim"), ROOT, REF]   # (ROOT first: `tests` is ours)

import numpy as np  # noqa: E402

import optiland.backend as be  # noqa: E402

from tests import _forbes as F  # noqa: E402


def _np(v):
    return np.asarray(be.to_numpy(v), dtype=np.float64).reshape(-1)


def backend(name: str):
    be.set_backend(name)
    if name == "torch":
        be.set_device("cpu")
        be.set_precision("float64")


def trace_rows(kind, variant, tol, rayset):
    """(S + 1, 8, n): what every surface recorded of one `SurfaceGroup.trace`."""
    lens = F.singlet(kind, variant, tol)
    hy, px, py = F.pupil_points(rayset)
    n = px.size
    rays = lens.ray_tracer.ray_generator.generate_rays(
        be.array(np.zeros(n)), be.array(np.full(n, hy)), be.array(px), be.array(py), F.WAVELENGTH)
    lens.surfaces.trace(rays)
    rows = []
    for s in lens.surfaces.surfaces:
        rows.append(np.stack([np.broadcast_to(_np(getattr(s, k)), (n,))
                              for k in ("x", "y", "z", "L", "M", "N", "intensity", "opd")]))
    return np.stack(rows)


def case_rows(kind, variant, tol, sets):
    return np.concatenate([trace_rows(kind, variant, tol, r) for r in sets], axis=2)


def maxdiff(a, b):
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN patterns differ"
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    return np.where(np.isnan(d), 0.0, d).max(axis=-1)


def grid_points(norm):
    ax = np.linspace(-1.2 * norm, 1.2 * norm, 33)
    gx, gy = np.meshgrid(ax, ax)
    extra = [norm * (1.0 + e) for e in (-1e-9, 1e-9, -2e-3, 2e-3)]
    x = np.concatenate([gx.reshape(-1), extra, np.zeros(4), [-v for v in extra]])
    y = np.concatenate([gy.reshape(-1), np.zeros(4), extra, np.zeros(4)])
    return x, y


def grid_values(kind, variant, x, y):
    geom = F.singlet(kind, variant).surfaces.surfaces[F.FORBES].geometry
    sag = _np(geom.sag(be.array(x), be.array(y)))
    nrm = np.stack([_np(v) for v in geom._surface_normal(be.array(x), be.array(y))])
    return sag, nrm


def main():
    out, names = {}, []
    worst = {"spread_pos": 0.0, "spread_opd": 0.0, "gap": 0.0, "default": 0.0}
    for kind in F.KINDS:
        for variant in F.VARIANTS:
            sets = F.RAYSETS + ((F.BIG_SET,) if variant == "norm8" else ())
            backend("numpy")
            table = F.packed(F.singlet(kind, variant, F.TIGHT))
            assert table.forbes == (F.FORBES,) and table.unsupported == (), (kind, variant)
            rows = {tol: case_rows(kind, variant, tol, sets)
                    for tol in (F.TIGHT, F.DEFAULT, F.TIGHTER)}
            backend("torch")
            torch_rows = {tol: case_rows(kind, variant, tol, sets) for tol in (F.TIGHT, F.DEFAULT)}
            backend("numpy")
            lo, bounds = 0, []
            for r in sets:
                n = F.pupil_points(r)[1].size
                bounds.append((r, lo, lo + n))
                lo += n
            tight_name = f"{kind}_{variant}_tight"
            for label, tol in (("tight", F.TIGHT), ("default", F.DEFAULT)):
                name = f"{kind}_{variant}_{label}"
                names.append(name)
                t = F.packed(F.singlet(kind, variant, tol))
                out[f"{name}/kind"], out[f"{name}/variant"] = np.array(kind), np.array(variant)
                out[f"{name}/tol"] = np.float64(tol)
                out[f"{name}/table"] = np.array(t.to_json())
                out[f"{name}/set_names"] = np.array([b[0] for b in bounds])
                out[f"{name}/set_lo"] = np.array([b[1] for b in bounds], dtype=np.int64)
                out[f"{name}/set_hi"] = np.array([b[2] for b in bounds], dtype=np.int64)
                out[f"{name}/spread"] = maxdiff(rows[tol], torch_rows[tol])
                if label == "tight":
                    out[f"{name}/rows"] = rows[tol]
                    out[f"{name}/gap"] = maxdiff(rows[F.TIGHT], rows[F.TIGHTER])
                    worst["gap"] = max(worst["gap"], float(out[f"{name}/gap"].max()))
                else:
                    d = rows[tol] - rows[F.TIGHT]
                    d = np.where(np.isnan(d), 0.0, d)
                    assert np.array_equal(np.isnan(rows[tol]), np.isnan(rows[F.TIGHT]))
                    out[f"{name}/tight"] = np.array(tight_name)
                    out[f"{name}/delta"] = d.astype(np.float32)
                    back = rows[F.TIGHT] + d.astype(np.float32).astype(np.float64)
                    assert float(maxdiff(back, rows[tol]).max()) < 1e-16
                    worst["default"] = max(worst["default"], float(np.abs(d).max()))
                sp = out[f"{name}/spread"]
                worst["spread_pos"] = max(worst["spread_pos"], float(sp[:, :6].max()))
                worst["spread_opd"] = max(worst["spread_opd"], float(sp[:, 7].max()))
            # what may be NaN: nothing in these cases (every ray reaches every surface)
            assert not np.isnan(rows[F.TIGHT][:, :6]).any(), (kind, variant)
            if variant == "clipped":
                assert (rows[F.TIGHT][F.FORBES, 6] == 0.0).any(), "the aperture clips nothing"
            if kind == "q2d":
                edge = F.near_edge(table, rows[F.TIGHT])
                assert edge.mean() <= F.EDGE_CAP, (kind, variant, float(edge.mean()))
            p = F.local_hit(table, rows[F.TIGHT])
            u = np.hypot(p[0], p[1]) / float(table.surfaces[F.FORBES]["norm_radius"])
            if variant == "norm8":
                assert (u < 1).any() and (u > 1).any()
            if variant == "norm12":
                assert (u < 1).all()
            print(f"{kind}_{variant}: n={rows[F.TIGHT].shape[2]} u in [{u.min():.3f}, {u.max():.3f}]",
                  flush=True)
        for variant in ("norm12", "flat"):
            backend("numpy")
            lens = F.singlet(kind, variant)
            norm = float(_np(lens.surfaces.surfaces[F.FORBES].geometry.norm_radius)[0])
            x, y = grid_points(norm)
            sag, nrm = grid_values(kind, variant, x, y)
            table = F.packed(lens)
            backend("torch")
            t_sag, t_nrm = grid_values(kind, variant, x, y)
            backend("numpy")
            pre = f"grid_{kind}_{variant}/"
            out[pre + "table"] = np.array(table.to_json())
            out[pre + "x"], out[pre + "y"] = x, y
            out[pre + "sag"], out[pre + "normal"] = sag, nrm
            keep = np.ones(x.size, dtype=bool)
            if kind == "q2d":
                keep = np.abs(np.hypot(x, y) / norm - 1.0) >= F.EDGE
            out[pre + "sag_spread"] = np.float64(maxdiff(sag[keep], t_sag[keep]))
            out[pre + "normal_spread"] = np.float64(maxdiff(nrm[:, keep], t_nrm[:, keep]).max())
            print(f"{pre} sag spread {float(out[pre + 'sag_spread']):.2e} normal spread "
                  f"{float(out[pre + 'normal_spread']):.2e}", flush=True)
    out["cases"] = np.array(names)
    print("worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    np.savez_compressed(F.GOLD, **out)
    size = os.path.getsize(F.GOLD)
    print(f"{F.GOLD}: {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
