"""Shared pieces of the Huygens PSF tests: the golden fixture (tools/make_golden_huygens.py)
and a NumPy fp64 restatement of the reference's Huygens-Fresnel sum
(psf/huygens_fresnel_strategies.py:124-172), the yardstick of `ol_huygens_psf`."""

from __future__ import annotations

import os

import numpy as np

from tests._util import GOLDEN

ARGS = ("image_x", "image_y", "image_z", "pupil_x", "pupil_y", "pupil_z", "pupil_amp",
        "pupil_opd", "wavelength", "Rp")
SYSTEMS = {"cooke": "cooke_generic", "dgauss": "double_gauss"}


def golden():
    return dict(np.load(os.path.join(GOLDEN, "huygens.npz")))


def cases(g=None):
    g = golden() if g is None else g
    return [str(c) for c in g["cases"]]


def calls(g, case):
    """[(args tuple in compute() order, output)] of every compute() call of a case."""
    out = []
    for k in range(int(g[f"{case}/n_calls"])):
        args = tuple(g[f"{case}/call{k}/{a}"] for a in ARGS)
        out.append((args, g[f"{case}/call{k}/out"]))
    return out


def direct_field(image_x, image_y, image_z, pupil_x, pupil_y, pupil_z, amp, opd, wavelength,
                 Rp, block=256):
    """The complex field of the reference's sum, term for term, in fp64 (image-shaped)."""
    k = 2.0 * np.pi / float(wavelength)
    Rp = float(Rp)
    ix, iy, iz = (np.asarray(v, dtype=np.float64).reshape(-1, 1)
                  for v in (image_x, image_y, image_z))
    px, py, pz = (np.asarray(v, dtype=np.float64).reshape(1, -1)
                  for v in (pupil_x, pupil_y, pupil_z))
    a = np.asarray(amp).reshape(1, -1)
    w = a * np.exp(-1j * k * np.asarray(opd, dtype=np.float64).reshape(1, -1))
    field = np.empty(ix.shape[0], dtype=np.complex128)
    for s in range(0, ix.shape[0], block):
        dx, dy, dz = ix[s:s + block] - px, iy[s:s + block] - py, iz[s:s + block] - pz
        R = np.sqrt(dx * dx + dy * dy + dz * dz)
        q = 0.5 * (1.0 + (dx * px / Rp + dy * py / Rp + dz * pz / Rp) / R)
        field[s:s + block] = (w * np.exp(1j * k * R) / R * q).sum(axis=1)
    return field.reshape(np.shape(image_x))


def direct_sum(*args, **kwargs):
    """|field|^2 of `direct_field`."""
    f = direct_field(*args, **kwargs)
    return f.real ** 2 + f.imag ** 2


def random_case(n_pupil, n_image, complex_amp=False, seed=0):
    """Pupil samples on a cap of the reference sphere (Rp 54 mm, a 10 mm pupil) and image
    points within 25 um of the focus 60 mm away -- the geometry of the golden Cooke case."""
    rng = np.random.default_rng(seed)
    r = 4.8 * np.sqrt(rng.random(n_pupil))
    th = 2 * np.pi * rng.random(n_pupil)
    px, py = r * np.cos(th), r * np.sin(th)
    pz = 6.08 + (54.09 - np.sqrt(54.09 ** 2 - px * px - py * py))
    amp = 0.5 + 0.5 * rng.random(n_pupil)
    if complex_amp:
        amp = amp * np.exp(1j * 2 * np.pi * rng.random(n_pupil))
    opd = 1e-3 * rng.standard_normal(n_pupil)
    ix = 0.025 * (2 * rng.random(n_image) - 1)
    iy = 0.1 + 0.025 * (2 * rng.random(n_image) - 1)
    iz = 60.17675 + 1e-3 * rng.standard_normal(n_image)
    return ix, iy, iz, px, py, pz, amp, opd, 5.5e-4, 54.09227667996531
