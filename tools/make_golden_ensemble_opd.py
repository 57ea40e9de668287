#!/usr/bin/env python
"""tests/golden/ensemble_opd.npz: the wavefronts of K = 6 variants of two lenses from the reference
on its NumPy backend in fp64, for tests/test_ensemble_opd_cpu.py, tests/test_gpu_ensemble_opd.py
and tests/test_gpu_tolerancing_opd.py.  Lenses, variants, fields and wavelengths are those of
tests/_ensemble.py, unchanged; the layout of the file: tests/_ensemble_opd.py.

Per variant: the perturbations are applied, the optic is packed (`pack_optic`, strict), and for
every (field, wavelength) OPD, intensity and radius of `Wavefront(optic, [(hx, hy)], [w], 5,
"hexapolar")` are kept and `RayOperand.OPD_difference(optic, hx, hy, 3, w)` is evaluated (its
default Gaussian quadrature: 3 points on axis, 9 off axis; the points and weights of the
reference's `GaussianQuadrature` are kept too).

The aspheric singlet's Newton `tol` is set to 1e-12 on the reference geometry BEFORE packing and
tracing: the factory's 1e-6 mm is 2e-3 waves of batch-wide stop rule (tests/test_wavefront.py),
and the packed tables then carry the tight tolerance.

Asserted here: all 24 (lens, variant, field) combinations give finite OPD at the lens's first
wavelength; the tilted + decentred Cooke variant keeps 85 of 91 rays at field 0.7 and the other 23
combinations keep all 91; the radius-in-front-of-the-stop variant's entrance pupil is not the
nominal one (its EPD and exit pupil are: see `lens_block`) and the thickness variant's exit-pupil
position is not; every variant passes the ensemble's structure check.

    python tools/make_golden_ensemble_opd.py        (needs the reference package; CPU only)
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
from tests import _ensemble_opd as EO  # noqa: E402


def _np(v):
    return np.asarray(be.to_numpy(v), dtype=np.float64).reshape(-1)


def build_lens(name: str):
    optic = E.build_lens(name)
    if name == "singlet":
        optic.surfaces.surfaces[1].geometry.tol = EO.SINGLET_NEWTON_TOL
    return optic


def quadrature() -> dict:
    from optiland.distribution import GaussianQuadrature
    out = {}
    for key, sym, rep in (("gq_axis", True, 1), ("gq_field", False, 3)):
        d = GaussianQuadrature(is_symmetric=sym)
        d.generate_points(num_rings=EO.OPERAND_RINGS)
        out[f"{key}/px"], out[f"{key}/py"] = _np(d.x), _np(d.y)
        out[f"{key}/weights"] = np.repeat(_np(d.get_weights(EO.OPERAND_RINGS)), rep)
    return out


def lens_block(name: str) -> dict:
    from optiland.distribution import create_distribution
    from optiland.optimization.operand.ray import RayOperand
    from optiland.wavefront import Wavefront

    fields, wls = E.FIELDS[name], E.WAVELENGTHS[name]
    d = create_distribution("hexapolar")
    d.generate_points(E.RINGS)
    px, py = _np(d.x), _np(d.y)
    assert px.size == E.N_RAYS
    K, F, W = len(E.VARIANTS[name]), len(fields), len(wls)
    opd = np.zeros((K, F, W, E.N_RAYS))
    inten = np.zeros((K, F, W, E.N_RAYS))
    radius = np.zeros((K, F, W))
    operand = np.zeros((K, F, W))
    tables = []
    for k, (_label, recipe) in enumerate(E.VARIANTS[name]):
        optic = build_lens(name)     # a fresh optic per variant, as make_golden_ensemble.py
        for p in E.perturbations(optic, recipe):
            p.apply()
        tables.append(pack_optic(optic, list(wls)))
        for fi, (hx, hy) in enumerate(fields):
            for wi, w in enumerate(wls):
                data = Wavefront(optic, [(hx, hy)], [w], E.RINGS, "hexapolar").get_data((hx, hy), w)
                opd[k, fi, wi], inten[k, fi, wi] = _np(data.opd), _np(data.intensity)
                radius[k, fi, wi] = float(_np(data.radius)[0])
                operand[k, fi, wi] = float(RayOperand.OPD_difference(optic, hx, hy,
                                                                     EO.OPERAND_RINGS, w))
    check_structure(tables)
    if name == "singlet":
        t = tables[0].surfaces
        assert (t["tol"][t["max_iter"] > 0] == EO.SINGLET_NEWTON_TOL).all(), t["tol"]
    kept = (inten[:, :, 0] > 0).sum(axis=-1)          # (K, F) at the first wavelength
    assert np.isfinite(opd[:, :, 0]).all(), f"{name}: a non-finite OPD at the first wavelength"
    want = np.full((K, F), E.N_RAYS)
    if name == "cooke":
        want[E.CLIPPED_VARIANT, 1] = EO.CLIPPED_KEPT
    assert (kept == want).all(), f"{name}: rays kept {kept.tolist()}"
    # The radius in front of the stop moves the ENTRANCE pupil only: both lenses state their
    # aperture as an entrance-pupil diameter and the exit pupil is the stop's image through what
    # lies BEHIND it, so that variant's EPD and pupil_z are the nominal ones.  What a cell carries
    # per variant moves with the thickness variant (the image plane, hence pupil_z, shifts).
    a, b = tables[E.RADIUS_VARIANT].raygen, tables[0].raygen
    assert a["EPL"] != b["EPL"], f"{name}: the entrance pupil did not move"
    assert tables[EO.THICKNESS_VARIANT].raygen["pupil_z"] != b["pupil_z"], \
        f"{name}: no variant carries an exit pupil of its own"
    print(name, "rays kept (variant, field):", kept.tolist(), "pupil_z:",
          [round(t.raygen["pupil_z"], 6) for t in tables])
    return {f"{name}/tables": np.array([t.to_json() for t in tables]),
            f"{name}/fields": np.asarray(fields, dtype=np.float64),
            f"{name}/wavelengths": np.asarray(wls, dtype=np.float64),
            f"{name}/px": px, f"{name}/py": py, f"{name}/opd": opd, f"{name}/intensity": inten,
            f"{name}/radius": radius, f"{name}/operand": operand}


def main():
    out = quadrature()
    for name in E.LENSES:
        out.update(lens_block(name))
    np.savez_compressed(EO.GOLD, **out)
    size = os.path.getsize(EO.GOLD)
    assert size < (1 << 20), size
    print(EO.GOLD, size, "bytes")


if __name__ == "__main__":
    main()
