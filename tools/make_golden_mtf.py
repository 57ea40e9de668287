#!/usr/bin/env python
"""tests/golden/geometric_mtf.npz: the reference's `GeometricMTF` (mtf/geometric.py:27-204) and
`FFTMTF` (mtf/fft.py:19-235) on its NumPy backend (CPU, fp64), for tests/test_*geometric_mtf*.py.

Per geometric case: `freq`, `cutoff_freq`, `max_freq`, `diff_limited_mtf`, `mtf` (fields, 2,
num_points: [tangential, sagittal]) and, per field, the hits `x`, `y` and `np.histogram`'s
counts and edges of both curves.  Cases that share a lens, `num_rays` and `distribution` share
their hits (`hits_of`).  Per case also `fp32_spread`: the largest change of the reference's own
MTF of that case when its hits are jittered by a Gaussian of 6e-6 mm (the documented parity of
the fp32 tracer) -- the yardstick of the fp32 stand-alone test -- and `fp64_spread`, the same at
1e-9 mm.  Per FFT case: `mtf` (fields, 2, grid_size // 2), `freq_tang`, `freq_sag`.

    python tools/make_golden_mtf.py          (needs the reference package; CPU only)
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
from optiland.mtf import FFTMTF, GeometricMTF  # noqa: E402
from optiland.samples.objectives import CookeTriplet, DoubleGauss  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "geometric_mtf.npz")
LENS = {"cooke": CookeTriplet, "dgauss": DoubleGauss}

# name -> (lens, keyword arguments); every case: all fields, primary wavelength
CASES = {
    "cooke": ("cooke", {}),
    "dgauss": ("dgauss", {}),
    "cooke_n64": ("cooke", {"num_points": 64}),
    "cooke_f100": ("cooke", {"max_freq": 100.0}),
    "cooke_noscale": ("cooke", {"scale": False}),
    "cooke_hex12": ("cooke", {"distribution": "hexapolar", "num_rays": 12}),
    "dgauss_hex12": ("dgauss", {"distribution": "hexapolar", "num_rays": 12}),
}
FFT_CASES = {
    "fft_cooke": ("cooke", {"num_rays": 32, "grid_size": 64}),
    "fft_dgauss": ("dgauss", {"num_rays": 32, "grid_size": 64}),
    "fft_cooke_f50": ("cooke", {"num_rays": 32, "grid_size": 64, "max_freq": 50.0}),
}
JITTER_FP32_MM, JITTER_FP64_MM = 6e-6, 1e-9


def _np(v):
    return np.asarray(be.to_numpy(v), dtype=np.float64)


def _spread(m, sigma, seed=0):
    """max |MTF(hits + N(0, sigma)) - MTF(hits)| over every curve and frequency."""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for fd, mt in zip(m.data, m.mtf):
        for arr, ref in ((fd[0].y, mt[0]), (fd[0].x, mt[1])):
            a = _np(arr)
            got = m._compute_field_data(a + rng.normal(0.0, sigma, a.shape), m.freq,
                                        m.diff_limited_mtf)
            worst = max(worst, float(np.abs(_np(got) - _np(ref)).max()))
    return worst


def main():
    be.set_backend("numpy")
    out = {"cases": np.array(list(CASES)), "fft_cases": np.array(list(FFT_CASES))}
    hits_of = {}
    for name, (lens, kw) in CASES.items():
        m = GeometricMTF(LENS[lens](), **kw)
        key = (lens, kw.get("num_rays", 100), kw.get("distribution", "uniform"))
        owner = hits_of.setdefault(key, name)
        out[f"{name}/system"] = np.array(lens)
        out[f"{name}/hits_of"] = np.array(owner)
        out[f"{name}/num_rays"] = np.int64(key[1])
        out[f"{name}/distribution"] = np.array(key[2])
        out[f"{name}/num_points"] = np.int64(m.num_points)
        out[f"{name}/max_freq_in"] = np.float64(kw.get("max_freq", np.nan))
        out[f"{name}/scale"] = np.bool_(kw.get("scale", True))
        out[f"{name}/wavelength"] = np.float64(m.wavelengths[0].value)
        out[f"{name}/fields"] = np.array([[float(c) for c in f.coord] for f in m.fields])
        out[f"{name}/freq"] = _np(m.freq)
        out[f"{name}/cutoff_freq"] = np.float64(_np(m.cutoff_freq))
        out[f"{name}/max_freq"] = np.float64(_np(m.max_freq))
        out[f"{name}/diff_limited_mtf"] = _np(m.diff_limited_mtf)
        out[f"{name}/mtf"] = np.array([[_np(t), _np(s)] for t, s in m.mtf])
        for k, fd in enumerate(m.data):
            x, y = _np(fd[0].x), _np(fd[0].y)
            if owner == name:
                out[f"{name}/x{k}"], out[f"{name}/y{k}"] = x, y
            for tag, a in (("t", y), ("s", x)):   # tangential = y, sagittal = x
                counts, edges = np.histogram(a, bins=m.num_points + 1)
                out[f"{name}/counts_{tag}{k}"] = counts.astype(np.int32)
                out[f"{name}/edges_{tag}{k}"] = edges
        line = f"{name:14s} fields={len(m.data)} points={_np(m.data[0][0].x).size} " \
               f"cutoff={float(out[name + '/cutoff_freq']):.4f}"
        out[f"{name}/fp32_spread"] = np.float64(_spread(m, JITTER_FP32_MM))
        out[f"{name}/fp64_spread"] = np.float64(_spread(m, JITTER_FP64_MM))
        line += f" spread(6e-6 mm)={float(out[name + '/fp32_spread']):.3e}" \
                f" spread(1e-9 mm)={float(out[name + '/fp64_spread']):.3e}"
        print(line)
    for name, (lens, kw) in FFT_CASES.items():
        m = FFTMTF(LENS[lens](), **kw)
        out[f"{name}/system"] = np.array(lens)
        out[f"{name}/num_rays"] = np.int64(kw["num_rays"])
        out[f"{name}/grid_size"] = np.int64(kw["grid_size"])
        out[f"{name}/max_freq_in"] = np.float64(kw.get("max_freq", np.nan))
        out[f"{name}/max_freq"] = np.float64(_np(m.max_freq))
        out[f"{name}/mtf"] = np.array([[_np(t), _np(s)] for t, s in m.mtf])
        out[f"{name}/freq_tang"] = np.array([_np(f) for f in m.freq_tang])
        out[f"{name}/freq_sag"] = np.array([_np(f) for f in m.freq_sag])
        out[f"{name}/FNO"] = np.array([float(_np(f)) for f in m.FNO])
        print(f"{name:14s} fields={len(m.mtf)} max_freq={float(out[name + '/max_freq']):.4f}")
    np.savez_compressed(GOLD, **out)
    print(f"{GOLD}: {os.path.getsize(GOLD)} bytes")


if __name__ == "__main__":
    main()
