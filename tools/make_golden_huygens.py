#!/usr/bin/env python
"""tests/golden/huygens.npz: the reference's scalar Huygens PSF (psf/huygens_fresnel.py:31-348)
on its torch backend (CPU, fp64), for the Huygens tests (tests/test_huygens_*.py).

For every case it stores the inputs and output of each `compute()` call the reference made
(the PSF itself, then the ideal-pupil normalisation at one image point) and the final `psf`,
`strehl_ratio()`, `pixel_pitch`, `cx`, `cy`, `normalization`.

    python tools/make_golden_huygens.py          (needs the reference package; CPU only)
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
from optiland.psf import huygens_fresnel_strategies as strategies  # noqa: E402
from optiland.psf.huygens_fresnel import ScalarHuygensPSF  # noqa: E402
from optiland.samples.objectives import CookeTriplet, DoubleGauss  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "huygens.npz")
ARGS = ("image_x", "image_y", "image_z", "pupil_x", "pupil_y", "pupil_z", "pupil_amp",
        "pupil_opd", "wavelength", "Rp")

# name -> (system, field, wavelength, extra keyword arguments); num_rays 32, image_size 32
CASES = {
    "cooke_00": ("cooke", (0.0, 0.0), 0.55, {}),
    "cooke_01": ("cooke", (0.0, 1.0), 0.55, {}),
    "dgauss_007": ("dgauss", (0.0, 0.7), 0.5876, {}),
    "cooke_01_oversample": ("cooke", (0.0, 1.0), 0.55, {"oversample": 2.0}),
    "dgauss_007_pitch": ("dgauss", (0.0, 0.7), 0.5876, {"pixel_pitch": 0.0015}),
}


def _np(v):
    return np.asarray(be.to_numpy(v), dtype=np.float64)


def main():
    be.set_backend("torch")
    be.set_device("cpu")
    be.set_precision("float64")
    calls = []
    original = strategies.TorchSummation.compute

    def recording(self, *args):
        out = original(self, *args)
        calls.append([_np(a) for a in args] + [_np(out)])
        return out

    strategies.TorchSummation.compute = recording
    out = {"cases": np.array(list(CASES))}
    try:
        for name, (system, field, wl, extra) in CASES.items():
            calls.clear()
            optic = CookeTriplet() if system == "cooke" else DoubleGauss()
            psf = ScalarHuygensPSF(optic, field, wl, num_rays=32, image_size=32, **extra)
            out[f"{name}/system"] = np.array(system)
            out[f"{name}/field"] = np.array(field, dtype=np.float64)
            out[f"{name}/wavelength"] = np.float64(wl)
            out[f"{name}/oversample"] = np.float64(extra.get("oversample", np.nan))
            out[f"{name}/pixel_pitch_in"] = np.float64(extra.get("pixel_pitch", np.nan))
            out[f"{name}/psf"] = _np(psf.psf)
            out[f"{name}/strehl"] = np.float64(psf.strehl_ratio())
            out[f"{name}/pixel_pitch"] = np.float64(_np(psf.pixel_pitch))
            out[f"{name}/cx"] = np.float64(_np(psf.cx))
            out[f"{name}/cy"] = np.float64(_np(psf.cy))
            out[f"{name}/normalization"] = np.float64(_np(psf.normalization))
            out[f"{name}/n_calls"] = np.int64(len(calls))
            for k, call in enumerate(calls):
                for arg, v in zip(ARGS + ("out",), call):
                    out[f"{name}/call{k}/{arg}"] = v
            print(f"{name:22s} strehl={float(out[name + '/strehl']):.6f} "
                  f"pitch={float(out[name + '/pixel_pitch']):.3e} calls={len(calls)} "
                  f"pupil={calls[0][3].size}")
    finally:
        strategies.TorchSummation.compute = original
    np.savez_compressed(GOLD, **out)
    print(f"{GOLD}: {os.path.getsize(GOLD)} bytes")


if __name__ == "__main__":
    main()
