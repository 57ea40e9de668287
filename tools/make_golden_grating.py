#!/usr/bin/env python
"""tests/golden/grating.npz: the reference's diffraction gratings (geometries/plane_grating.py,
geometries/standard_grating.py, interactions/diffractive_model.py, RealRays.gratingdiffract)
traced by its own `SurfaceGroup.trace` on the NumPy backend (CPU, fp64), for
tests/test_grating_cpu.py and tests/test_gpu_grating.py.  Lenses, variants and ray sets are
tests/_grating.py's (`CASES`): the three lenses of the reference's tests/test_grating.py, groove
angle 0.6, orders -2 / 0 / +1, a grating between two glasses, a tilted and decentred one, a
clipping aperture, a SimpleCoating, and two evanescent cases (period 0.7 um, order -+1, field at
the edge).  Per case:

  table                  the packed table (JSON text, `pack_surfaces(tolerate=True, gratings=True)`)
  g                      index of the grating row
  rows (S + 1, 8, n)     every recorded row of the 127-ray hexapolar set, x y z L M N intensity opd
                         (row 0 is the object surface's: the input rays): the state in front of
                         the grating is row g - 1, its recorded row is row g
  big_in, big_out (8, m) BIG_CASES only: rows g - 1 and g of the 1027-ray set
and `known_*`: the known answers of the reference's tests/test_grating.py as data -- per ray the
state in front of the grating (`known_in`, (7, 8)), the lens (`known_lens`), the expected direction
triple behind it (`known_LMN`, the constants of that file) and what the reference traced
(`known_out`, (7, 8)).

Rays with |S| / n2^2 < 1e-2 (tests/_grating.radicand) are dropped before saving.  Asserted here:
the margin, 10-90 % NaN directions in the evanescent cases and none elsewhere, clipped rays in
the clipped case, the known answers to rtol 1e-5 / atol 1e-7.

    python tools/make_golden_grating.py        (needs the reference package; CPU only)
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

from tests import _grating as G  # noqa: E402

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


def main():
    be.set_backend("numpy")
    out, names = {}, []
    for name, (base, _edit, hy) in G.CASES.items():
        optic = G.case_lens(name)
        table = G.packed(optic)
        g = G.grating_index(base)
        assert table.gratings == (g,) and table.unsupported == (), (name, table.unsupported)
        sets = {"hex127": trace_rows(optic, 0.0, hy, *G.pupil_points("hex127"))}
        if name in G.BIG_CASES:
            sets[G.BIG_SET] = trace_rows(optic, 0.0, hy, *G.pupil_points(G.BIG_SET))
        evan = name.startswith("evan")
        for key, rows in list(sets.items()):
            s = G.radicand(table, g, rows[g - 1], rows[g])
            keep = np.abs(s) >= G.MARGIN
            rows = sets[key] = rows[:, :, keep]
            s = s[keep]
            nan = np.isnan(rows[g, 3])
            assert np.array_equal(nan, s < 0), name          # NaN exactly where S < 0 ...
            assert not np.isnan(rows[g, :3]).any(), name     # ... and the position stays finite
            if evan:
                assert 0.1 <= nan.mean() <= 0.9, (name, float(nan.mean()))
            else:
                assert not np.isnan(rows).any(), name
            print(f"{name} {key}: kept {int(keep.sum())} of {keep.size}, NaN {nan.mean():.2f}, "
                  f"min |S|/n2^2 {np.abs(s).min():.3g}", flush=True)
        if name == "clipped":
            hit = sets["hex127"][g, 6] == 0.0
            assert hit.any() and not hit.all(), "the aperture clips nothing / everything"
        names.append(name)
        out[f"{name}/table"] = np.array(table.to_json())
        out[f"{name}/g"] = np.int64(g)
        out[f"{name}/rows"] = sets["hex127"]
        if name in G.BIG_CASES:
            out[f"{name}/big_in"] = sets[G.BIG_SET][g - 1]
            out[f"{name}/big_out"] = sets[G.BIG_SET][g]

    k_in, k_out, k_lmn, k_lens = [], [], [], []
    for base, (hx, hy, px, py), lmn in G.KNOWN:
        optic = G.lens(base)
        optic.updater.update_paraxial()
        ray = optic.trace_generic(Hx=hx, Hy=hy, Px=px, Py=py, wavelength=G.WAVELENGTH)
        got = [float(_np(v)[0]) for v in (ray.L, ray.M, ray.N)]
        np.testing.assert_allclose(got, lmn, rtol=1e-5, atol=1e-7)
        rows = recorded(optic, 1)
        g = G.grating_index(base)
        # behind the grating the ray only meets the image plane: the direction there is final
        np.testing.assert_allclose(rows[g, 3:6, 0], got, rtol=0, atol=1e-15)
        k_in.append(rows[g - 1, :, 0])
        k_out.append(rows[g, :, 0])
        k_lmn.append(lmn)
        k_lens.append({"flat": "flat_t", "conic": "conic_t", "mirror": "conic_r"}[base])
    out["known_in"], out["known_out"] = np.array(k_in), np.array(k_out)
    out["known_LMN"], out["known_lens"] = np.array(k_lmn), np.array(k_lens)
    out["cases"] = np.array(names)
    np.savez_compressed(G.GOLD, **out)
    size = os.path.getsize(G.GOLD)
    print(f"{G.GOLD}: {size} bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
