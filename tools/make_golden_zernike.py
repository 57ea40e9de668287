#!/usr/bin/env python
"""tests/golden/zernike_fit.npz: the reference's `ZernikeFit` (zernike/fit.py:33-118) and
`SampledMTF` (mtf/sampled.py:17-207) on CPU at fp64, for tests/test_*zernike_fit*.py.

Index tables: `indices/<kind>` (120, 2) = (n, m) and `norms/<kind>` (120,) of the three schemes.

Samplings (`samp/<name>/x, y, z`): the Cooke triplet's OPD map at field (0, 0.7), primary
wavelength, over hexapolar pupils of 1, 6 and 15 rings (7, 127, 721 points) and the uniform grid
of `num_rays` 32 (740 points).

Fit cases (`fit_cases`; `<case>/sampling, kind, num_terms`): `coeffs`, the NumPy backend's
coefficients; `cond`, cond_2 of the design matrix (asserted <= 100: every case is full rank);
`spread`, the largest coefficient difference between the NumPy backend and the torch backend
(CPU, float64) on the same stored inputs -- `gamma` against `lgamma.exp`, two `lstsq` drivers.

Sampled-MTF cases from given inputs (`smtf_cases`): `x, y, opd, intensity, coeffs`, `kind`,
`shifts` (F, 2), `mtf` (NumPy backend) and `spread`, NumPy against torch-CPU on those inputs.

Sampled-MTF cases end to end (`e2e_cases`; `<case>/system, field, wavelength, num_rays`):
`freqs` (F, 2), `mtf` (NumPy backend) and `spread`, the larger of NumPy against torch-CPU end to
end and of the reference's own change when its OPD map is jittered by a Gaussian of 2e-10 waves
(the documented OPD parity of the fp64 trace); both figures are stored too.

    python tools/make_golden_zernike.py          (needs the reference package; CPU only)
"""

from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("OPTILAND_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.join(ROOT, "tests", "refshim"), REF, ROOT]

import numpy as np  # noqa: E402

import optiland.backend as be  # noqa: E402
from optiland.mtf import SampledMTF  # noqa: E402
from optiland.samples.objectives import CookeTriplet, DoubleGauss  # noqa: E402
from optiland.wavefront import Wavefront  # noqa: E402
from optiland.zernike import ZernikeFit, ZernikeFringe, ZernikeNoll, ZernikeStandard  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "zernike_fit.npz")
LENS = {"cooke": CookeTriplet, "dgauss": DoubleGauss}
KINDS = {"fringe": ZernikeFringe, "standard": ZernikeStandard, "noll": ZernikeNoll}
MAX_TERMS = 120
FIELD = (0.0, 0.7)
SAMPLINGS = {"hex1": ("hexapolar", 1), "hex6": ("hexapolar", 6), "hex15": ("hexapolar", 15),
             "uni32": ("uniform", 32)}
TERMS = {"hex1": (4,), "hex6": (37,), "hex15": (37, 120), "uni32": (37, 120)}
JITTER_WAVES = 2e-10
# name -> (lens, field, num_rays, kind, frequencies)
_AXIS = [(0.0, float(f)) for f in np.linspace(0.0, 80.0, 27)] + \
        [(float(f), 0.0) for f in (10.0, 40.0)] + [(7.0, 9.0), (-12.0, 5.0), (30.0, -30.0),
                                                   (400.0, 0.0)]
SMTF = {"cooke_fringe": ("cooke", FIELD, 32, "fringe", _AXIS),
        "dgauss_standard": ("dgauss", (0.0, 1.0), 24, "standard", _AXIS[:9] + _AXIS[-4:]),
        "cooke_noll_one": ("cooke", (0.0, 0.0), 16, "noll", [(0.0, 25.0)])}
E2E = {"cooke_n32": ("cooke", FIELD, 32), "cooke_n64": ("cooke", FIELD, 64),
       "dgauss_n32": ("dgauss", FIELD, 32)}
E2E_FREQS = [(0.0, float(f)) for f in np.linspace(0.0, 60.0, 13)] + \
            [(float(f), 0.0) for f in np.linspace(5.0, 60.0, 12)] + [(12.0, 16.0), (-20.0, 8.0)]


def _np(v):
    return np.asarray(be.to_numpy(v), dtype=np.float64)


def _backend(name):
    be.set_backend(name)
    if name == "torch":
        be.set_device("cpu")
        be.set_precision("float64")
        be.grad_mode.disable()


def _fit(x, y, z, kind, k):
    f = ZernikeFit(be.array(x), be.array(y), be.array(z), kind, k)
    return _np(f.coeffs), f


def _design(f):
    ones = type(f.zernike)(be.ones([f.num_terms]))
    return np.stack([_np(t) for t in ones.terms(f.radius, f.phi)], axis=1)


def _smtf_from(lens, field, num_rays, kind, given=None, terms=37):
    """A reference SampledMTF; with `given` = (x, y, opd, intensity, coeffs) its inputs replaced
    by the stored ones (what calculate_mtf reads: sampled.py:149-156)."""
    m = SampledMTF(LENS[lens](), field, "primary", num_rays=num_rays, zernike_terms=terms,
                   zernike_type=kind)
    if given is not None:
        x, y, opd, inten, coeffs = (be.array(v) for v in given)
        m.x_norm, m.y_norm, m.opd_waves, m.intensity = x, y, opd, inten
        m.zernike_fit.zernike.coeffs = coeffs
        m.P1 = be.sqrt(inten) * be.exp(1j * 2 * be.pi * opd)
        m.otf_at_zero = be.sum(inten)
    return m


def _mtf(m, freqs):
    return np.array([float(_np(v)) for v in m.calculate_mtf(freqs)])


def _shifts(m, freqs):
    wl_mm = float(m.wavelength) * 1e-3
    xpd, xpl = float(_np(m.xpd)), float(_np(m.xpl))
    return xpl * (wl_mm * np.asarray(freqs, dtype=np.float64)) / (xpd / 2)


def main():
    out = {}
    _backend("numpy")
    for kind, cls in KINDS.items():
        idx = cls._generate_indices(MAX_TERMS)
        out[f"indices/{kind}"] = np.array([[int(n), int(m)] for n, m in idx], dtype=np.int64)
        out[f"norms/{kind}"] = np.array([float(_np(cls._norm_constant(int(n), int(m))))
                                         for n, m in idx])
    lens = CookeTriplet()
    for name, (dist, num) in SAMPLINGS.items():
        w = lens.primary_wavelength
        wf = Wavefront(lens, fields=[FIELD], wavelengths=[w], num_rays=num, distribution=dist)
        d = wf.get_data(FIELD, w)
        assert bool(np.all(_np(d.intensity) > 0))
        out[f"samp/{name}/x"], out[f"samp/{name}/y"] = _np(wf.distribution.x), _np(wf.distribution.y)
        out[f"samp/{name}/z"] = _np(d.opd)
    fit_cases = []
    for name in SAMPLINGS:
        x, y, z = (out[f"samp/{name}/{k}"] for k in "xyz")
        for kind in KINDS:
            for k in TERMS[name]:
                case = f"{name}_{kind}_{k}"
                _backend("numpy")
                c_np, f = _fit(x, y, z, kind, k)
                cond = float(np.linalg.cond(_design(f)))
                assert cond <= 100.0, (case, cond)
                _backend("torch")
                c_t, _ = _fit(x, y, z, kind, k)
                spread = float(np.abs(c_np - c_t).max())
                fit_cases.append(case)
                out[f"{case}/sampling"], out[f"{case}/kind"] = np.array(name), np.array(kind)
                out[f"{case}/num_terms"] = np.int64(k)
                out[f"{case}/coeffs"], out[f"{case}/cond"] = c_np, np.float64(cond)
                out[f"{case}/spread"] = np.float64(spread)
                print(f"{case:22s} points={x.size} cond={cond:7.2f} max|c|={np.abs(c_np).max():.3f} "
                      f"spread={spread:.2e}")
    out["fit_cases"] = np.array(fit_cases)

    for case, (lname, field, num_rays, kind, freqs) in SMTF.items():
        _backend("numpy")
        m = _smtf_from(lname, field, num_rays, kind)
        given = tuple(_np(v) for v in (m.x_norm, m.y_norm, m.opd_waves, m.intensity,
                                       m.zernike_fit.coeffs))
        ref = _mtf(m, freqs)
        shifts = _shifts(m, freqs)
        _backend("torch")
        got = _mtf(_smtf_from(lname, field, num_rays, kind, given), freqs)
        spread = float(np.abs(ref - got).max())
        for key, v in zip(("x", "y", "opd", "intensity", "coeffs"), given):
            out[f"{case}/{key}"] = v
        out[f"{case}/kind"], out[f"{case}/shifts"] = np.array(kind), shifts
        out[f"{case}/mtf"], out[f"{case}/spread"] = ref, np.float64(spread)
        print(f"{case:22s} points={given[0].size} dark={int((given[3] <= 0).sum())} "
              f"freqs={len(freqs)} spread={spread:.2e}")
    out["smtf_cases"] = np.array(list(SMTF))

    for case, (lname, field, num_rays) in E2E.items():
        _backend("numpy")
        m = _smtf_from(lname, field, num_rays, "fringe")
        ref = _mtf(m, E2E_FREQS)
        rng = np.random.default_rng(0)
        x, y, opd, inten = (_np(v) for v in (m.x_norm, m.y_norm, m.opd_waves, m.intensity))
        opd_j = opd + rng.normal(0.0, JITTER_WAVES, opd.shape)
        c_j, _ = _fit(x, y, opd_j, "fringe", 37)
        jit = float(np.abs(_mtf(_smtf_from(lname, field, num_rays, "fringe",
                                           (x, y, opd_j, inten, c_j)), E2E_FREQS) - ref).max())
        _backend("torch")
        got = _mtf(_smtf_from(lname, field, num_rays, "fringe"), E2E_FREQS)
        backends = float(np.abs(ref - got).max())
        _backend("numpy")
        out[f"{case}/system"], out[f"{case}/field"] = np.array(lname), np.array(field)
        out[f"{case}/wavelength"] = np.float64(m.wavelength)
        out[f"{case}/num_rays"] = np.int64(num_rays)
        out[f"{case}/freqs"], out[f"{case}/mtf"] = np.array(E2E_FREQS), ref
        out[f"{case}/xpd"], out[f"{case}/xpl"] = np.float64(_np(m.xpd)), np.float64(_np(m.xpl))
        out[f"{case}/spread_backends"] = np.float64(backends)
        out[f"{case}/spread_jitter"] = np.float64(jit)
        out[f"{case}/spread"] = np.float64(max(backends, jit))
        print(f"{case:22s} points={x.size} backends={backends:.2e} jitter={jit:.2e}")
    out["e2e_cases"] = np.array(list(E2E))
    np.savez_compressed(GOLD, **out)
    print(f"{GOLD}: {os.path.getsize(GOLD)} bytes")


if __name__ == "__main__":
    main()
