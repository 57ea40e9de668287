#!/usr/bin/env python
"""tests/golden/ensemble.npz: K = 6 variants of two lenses traced by the reference on its NumPy
backend in fp64, for tests/test_ensemble_cpu.py and tests/test_gpu_ensemble.py.  Lenses, variants
(the reference's own `Perturbation` with fixed `ScalarSampler`s), fields, wavelengths and the
layout of the file: tests/_ensemble.py.

Per variant: the perturbations are applied, the optic is packed (`pack_optic`, strict), every
(field, wavelength) is traced with `Optic.trace(Hx, Hy, w, 5, "hexapolar")` and the image-plane
x, y, intensity are kept, `RayOperand.rms_spot_size` is evaluated, the perturbations are reset.

Asserted here: the nominal variant loses no ray; the radius-before-stop variant's entrance pupil
is NOT the nominal one (its packed EPL differs); the decentred Cooke variant loses rays in some
cell and keeps some in every cell; every variant passes the ensemble's structure check; after its
reset a variant's optic packs to the nominal table again (but where an index was perturbed: the
reference's reset leaves an ideal material behind, so every variant starts from a fresh optic).

    python tools/make_golden_ensemble.py        (needs the reference package; CPU only)
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

from optiland_amd.ensemble import check_structure  # noqa: E402
from optiland_amd.packer import pack_optic  # noqa: E402
from tests import _ensemble as E  # noqa: E402


def _np(v):
    return np.asarray(be.to_numpy(v), dtype=np.float64).reshape(-1)


def _same(a, b, tol=1e-12) -> bool:
    """Two packed tables agree to rounding (a thickness that is set and set back comes from
    differences of vertex positions: the last bit may move)."""
    def close(x, y):
        return np.allclose(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64),
                           rtol=tol, atol=tol, equal_nan=True)
    return all(close(a.surfaces[n], b.surfaces[n]) for n in a.surfaces.dtype.names) and \
        all(close(a.optics[n], b.optics[n]) for n in a.optics.dtype.names) and \
        close(a.coeffs, b.coeffs) and a.raygen.keys() == b.raygen.keys() and \
        all(close(a.raygen[k], b.raygen[k]) for k in a.raygen)


def lens_block(name: str) -> dict:
    from optiland.distribution import create_distribution
    from optiland.optimization.operand.ray import RayOperand

    fields, wls = E.FIELDS[name], E.WAVELENGTHS[name]
    d = create_distribution("hexapolar")
    d.generate_points(E.RINGS)
    px, py = _np(d.x), _np(d.y)
    assert px.size == E.N_RAYS
    K, F, W = len(E.VARIANTS[name]), len(fields), len(wls)
    hits = np.zeros((K, F, W, 3, E.N_RAYS))
    operand = np.zeros((K, F, W))
    tables, labels = [], []
    for k, (label, recipe) in enumerate(E.VARIANTS[name]):
        # a fresh optic per variant: the reference's reset of an index perturbation leaves an
        # ideal material behind (updater.set_index), which would leak into the later variants
        optic = E.build_lens(name)
        nominal = pack_optic(optic, list(wls))
        perts = E.perturbations(optic, recipe)
        for p in perts:
            p.apply()
        tables.append(pack_optic(optic, list(wls)))
        labels.append(label)
        for fi, (hx, hy) in enumerate(fields):
            for wi, w in enumerate(wls):
                optic.trace(hx, hy, w, E.RINGS, "hexapolar")
                sg = optic.surfaces
                hits[k, fi, wi] = [_np(sg.x[-1, :]), _np(sg.y[-1, :]), _np(sg.intensity[-1, :])]
                operand[k, fi, wi] = float(RayOperand.rms_spot_size(optic, -1, hx, hy, E.RINGS, w,
                                                                     "hexapolar"))
                assert abs(operand[k, fi, wi] - E.operand_from_hits(*hits[k, fi, wi, :2])) \
                    <= 1e-15 * max(1.0, operand[k, fi, wi]) or np.isnan(operand[k, fi, wi])
        for p in perts:
            p.reset()
        if not any(kind == "index" for kind, _v, _kw in recipe):
            again = pack_optic(optic, list(wls))
            assert _same(again, nominal), f"{name}: reset of variant {k} left the optic changed"
    check_structure(tables)
    alive = (hits[:, :, :, 2] > 0).sum(axis=-1)
    assert (alive[0] == E.N_RAYS).all(), f"{name}: the nominal variant loses rays {alive[0]}"
    assert tables[E.RADIUS_VARIANT].raygen["EPL"] != tables[0].raygen["EPL"], \
        f"{name}: the entrance pupil did not move"
    if name == "cooke":
        c = alive[E.CLIPPED_VARIANT]
        assert (c < E.N_RAYS).any() and (c > 0).all(), f"clipped variant keeps {c}"
    print(name, "rays kept per variant:", alive.reshape(K, -1).min(axis=1).tolist(),
          "EPL:", [round(t.raygen["EPL"], 6) for t in tables])
    return {f"{name}/tables": np.array([t.to_json() for t in tables]),
            f"{name}/labels": np.array(labels),
            f"{name}/fields": np.asarray(fields, dtype=np.float64),
            f"{name}/wavelengths": np.asarray(wls, dtype=np.float64),
            f"{name}/px": px, f"{name}/py": py,
            f"{name}/hits": hits, f"{name}/operand": operand}


def main():
    out = {}
    for name in E.LENSES:
        out.update(lens_block(name))
    np.savez_compressed(E.GOLD, **out)
    print(E.GOLD, os.path.getsize(E.GOLD), "bytes")


if __name__ == "__main__":
    main()
