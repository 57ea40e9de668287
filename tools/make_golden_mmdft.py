#!/usr/bin/env python
"""tests/golden/mmdft.npz: the reference's MMDFT PSF (psf/mmdft.py:19-283) on its NumPy backend
(CPU, fp64), for the MMDFT tests (tests/test_mmdft_cpu.py, tests/test_gpu_mmdft.py).

For every case it stores the constructor's arguments, the pupil (complex128), `pad_size` (the
expression of `_compute_kernels`), the resolved `num_rays`, `image_size`, `pixel_pitch`, the
working F/# at the case's field and wavelength, `psf`, `strehl_ratio()` and the count c of the
normalisation.  Besides: one `image_size > pad_size` request with the text of its ValueError, and
the parameter tables of the reference's own test_calcs_from_num_rays / _pixel_pitch /
_image_size (Cooke triplet, field (0, 0), 0.55 um) as the reference resolves them -- with
`_compute_psf` left out, which those numbers do not depend on.

    python tools/make_golden_mmdft.py          (needs the reference package; CPU only)
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
from optiland.psf.mmdft import MMDFTPSF  # noqa: E402
from optiland.samples.objectives import CookeTriplet, DoubleGauss  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "mmdft.npz")

# name -> (system, field, wavelength, num_rays, image_size, pixel_pitch, remove_tilt)
CASES = {
    "cooke_00": ("cooke", (0.0, 0.0), 0.55, 32, 32, None, False),
    "cooke_01_m48": ("cooke", (0.0, 1.0), 0.55, 32, 48, None, False),
    "dgauss_007_pitch": ("dgauss", (0.0, 0.7), 0.5876, 33, None, 0.9, False),
    "cooke_01_auto": ("cooke", (0.0, 1.0), 0.55, 64, None, None, False),
    "cooke_01_tilt": ("cooke", (0.0, 1.0), 0.55, 32, 32, None, True),
}
# an image larger than the pad size of its pitch: (system, field, wavelength, num_rays, image_size,
# pixel_pitch)
TOO_LARGE = ("cooke", (0.0, 0.0), 0.55, 32, 64, 2.0)
# the reference's tests/test_mmdft_psf.py: make_mmdftpsf(num_rays=..., image_size=None),
# (pixel_pitch=..., image_size=None) and (image_size=..., pixel_pitch=None), num_rays 128
FROM_NUM_RAYS = (32, 64, 128, 256, 1024)
FROM_PIXEL_PITCH = (0.25, 0.50, 0.75, 1.00, 1.50, 2.00)
FROM_IMAGE_SIZE = (128, 256, 512, 1024, 2048, 4096)


def _optic(system):
    return CookeTriplet() if system == "cooke" else DoubleGauss()


def _nan(v):
    return np.float64(np.nan if v is None else v)


def _resolved(num_rays, image_size, pixel_pitch):
    """(num_rays, image_size, pixel_pitch) as the reference's constructor resolves them."""
    psf = MMDFTPSF(CookeTriplet(), (0, 0), 0.55, num_rays=num_rays, image_size=image_size,
                   pixel_pitch=pixel_pitch)
    return [float(psf.num_rays), float(psf.image_size), float(psf.pixel_pitch)]


def main():
    be.set_backend("numpy")
    out = {"cases": np.array(list(CASES))}
    for name, (system, field, wl, num_rays, image_size, pitch, tilt) in CASES.items():
        psf = MMDFTPSF(_optic(system), field, wl, num_rays=num_rays, image_size=image_size,
                       pixel_pitch=pitch, remove_tilt=tilt)
        fno = float(psf._get_working_FNO())
        pad = float(psf.wavelengths[0].value * psf._get_working_FNO() * (psf.num_rays - 1)
                    / psf.pixel_pitch)
        out[f"{name}/system"] = np.array(system)
        out[f"{name}/field"] = np.array(field, dtype=np.float64)
        out[f"{name}/wavelength"] = np.float64(wl)
        out[f"{name}/num_rays_in"] = np.int64(num_rays)
        out[f"{name}/image_size_in"] = _nan(image_size)
        out[f"{name}/pixel_pitch_in"] = _nan(pitch)
        out[f"{name}/remove_tilt"] = np.bool_(tilt)
        out[f"{name}/pupil"] = np.asarray(psf.pupil, dtype=np.complex128)
        out[f"{name}/pad_size"] = np.float64(pad)
        out[f"{name}/num_rays"] = np.int64(psf.num_rays)
        out[f"{name}/image_size"] = np.int64(psf.image_size)
        out[f"{name}/pixel_pitch"] = np.float64(psf.pixel_pitch)
        out[f"{name}/working_fno"] = np.float64(fno)
        out[f"{name}/psf"] = np.asarray(psf.psf, dtype=np.float64)
        out[f"{name}/strehl"] = np.float64(psf.strehl_ratio())
        out[f"{name}/count"] = np.int64(np.sum(np.abs(psf.pupil) > 0))
        print(f"{name:18s} N={psf.num_rays} M={psf.image_size} pad={pad:.12f} "
              f"pitch={float(psf.pixel_pitch):.6f} strehl={float(psf.strehl_ratio()):.6f} "
              f"c={int(out[name + '/count'])}")

    system, field, wl, num_rays, image_size, pitch = TOO_LARGE
    try:
        MMDFTPSF(_optic(system), field, wl, num_rays=num_rays, image_size=image_size,
                 pixel_pitch=pitch)
        raise SystemExit("the too-large request did not raise")
    except ValueError as exc:
        out["too_large/system"] = np.array(system)
        out["too_large/field"] = np.array(field, dtype=np.float64)
        out["too_large/wavelength"] = np.float64(wl)
        out["too_large/request"] = np.array([num_rays, image_size, pitch], dtype=np.float64)
        out["too_large/error"] = np.array(str(exc))
        print(f"too_large: {exc}")

    stock = MMDFTPSF._compute_psf
    MMDFTPSF._compute_psf = lambda self: None   # (the tables are about the parameters alone)
    try:
        out["table/from_num_rays"] = np.array(
            [[n] + _resolved(n, None, None) for n in FROM_NUM_RAYS], dtype=np.float64)
        out["table/from_pixel_pitch"] = np.array(
            [[p] + _resolved(128, None, p) for p in FROM_PIXEL_PITCH], dtype=np.float64)
        out["table/from_image_size"] = np.array(
            [[m] + _resolved(128, m, None) for m in FROM_IMAGE_SIZE], dtype=np.float64)
    finally:
        MMDFTPSF._compute_psf = stock
    for key in ("from_num_rays", "from_pixel_pitch", "from_image_size"):
        print(f"table/{key} (request, num_rays, image_size, pixel_pitch):")
        print(out[f"table/{key}"])
    np.savez_compressed(GOLD, **out)
    print(f"{GOLD}: {os.path.getsize(GOLD)} bytes")


if __name__ == "__main__":
    main()
