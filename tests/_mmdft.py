"""Shared pieces of the MMDFT PSF tests: the golden fixtures (tools/make_golden_mmdft.py: the
reference's own `MMDFTPSF`; tools/make_golden_exact_mmdft.py: mpmath at 50 digits), a NumPy fp64
restatement of the reference's formula (psf/mmdft.py:157-283), and the bounds `ol_mmdft_psf` is
held to.

The bound against the EXACT transform -- rounding analysis of the kernel's own operations, no
measured figure.  With eps = 2^-52 (one ulp of 1) and u = eps / 2:

  table    W = exp(-2 pi i k / pad), k an exact integer.  The phase in cycles is the quotient
           t = fl(k / pad) and the remainder t_lo = fl((k - t pad) / pad), whose numerator one
           fma gives exactly; t - rint(t) is exact, and x = fl((t - rint t) + t_lo), |x| <= 1/2,
           is off by at most ulp(1/2) / 2 = 2^-55 cycles, that is 2 pi 2^-55 = 0.79 eps rad.
           sincospi is documented to 2 ulp: each of cos and sin, at most 1 in size, to 2 u 2 =
           eps, sqrt(2) eps for the pair.  An entry is within 0.79 eps + 1.42 eps <= 3 eps of
           the exact one: "good to 3 ulp".
  sums     acc <- acc + a b is four fmas: (re, im) <- fl(acc + a.re b), then (re, im) <-
           fl(that -/+ a.im (b.im, b.re)).  Each pair of roundings perturbs both components by
           a relative u at most, so the complex value by u times its modulus; the moduli are at
           most the sum of |a_i| |b_i| so far.  N terms: 2 N u = N eps times sum |a| |b|.
  G        T = g W^T: the table's 3 eps and the sum's N eps, times S_y = sum_x |g[y][x]| (|W| =
           1).  G = W T: the error of T carried through (sum_y of it), the table's 3 eps and
           the sum's N eps times sum_y |T[y][u]| <= sum |g|.  Together (2 N + 6) eps sum |g|.
  epilogue |G|^2 * 100 / c^2: an fma, a product, a product and a division, 4 u = 2 eps
           relative to the PSF, what an error of eps |G| <= eps sum |g| in G would give: + 1.
  fixture  the exact G and PSF are themselves rounded to fp64 once (u each): + 1.

  B = (2 N + 8) eps sum |g|         |G_dev - G_exact| <= B
                                    |psf_dev - psf_exact| <= (2 |G_exact| B + B^2) 100 / c^2

Against the REFERENCE's recorded outputs (mmdft.npz) the tolerance is that PSF form plus the
reference's own distance from the exact transform: its phase fl(fl(fl(2 pi) k) / pad) carries
three roundings of an argument of up to 1e4 rad that the kernel's does not.  `REFERENCE_ERROR`
is that distance as tools/make_golden_exact_mmdft.py measures it ON THE CPU -- the NumPy formula
(`direct`) against mpmath on the same inputs, the largest |psf - psf_exact| / max(psf_exact) over
the cases of exact_mmdft.npz -- and the tolerance takes it twice.  The kernel's results never
entered it.  (For orientation: the reference's NumPy and torch-CPU backends differ by 6e-12 of
the peak on the first case of mmdft.npz.)"""

from __future__ import annotations

import os

import numpy as np

from tests._util import GOLDEN

EPS = 2.0 ** -52
TABLE_ULP = 3
SYSTEMS = {"cooke": "cooke_generic", "dgauss": "double_gauss"}
# printed by tools/make_golden_exact_mmdft.py ("reference error: 4.840e-15 of the peak (case
# n64_m33)"); rounded up to two digits
REFERENCE_ERROR = 4.9e-15


def golden():
    return dict(np.load(os.path.join(GOLDEN, "mmdft.npz")))


def exact():
    return dict(np.load(os.path.join(GOLDEN, "exact_mmdft.npz")))


def cases(g):
    return [str(c) for c in g["cases"]]


def kwargs(g, case):
    """The constructor's (num_rays, image_size, pixel_pitch, remove_tilt) of a golden case."""
    size, pitch = float(g[f"{case}/image_size_in"]), float(g[f"{case}/pixel_pitch_in"])
    return dict(num_rays=int(g[f"{case}/num_rays_in"]),
                image_size=None if np.isnan(size) else int(size),
                pixel_pitch=None if np.isnan(pitch) else pitch,
                remove_tilt=bool(g[f"{case}/remove_tilt"]))


def kernel(n, m, pad):
    """The reference's left kernel (mmdft.py:266-282), operation for operation: (m, n)."""
    cp = np.arange(n) - n // 2
    ci = np.arange(m) - m // 2
    return np.exp(-2j * np.pi * np.outer(ci, cp) / pad).astype(np.complex128)


def direct_field(pupil, pad, m):
    """G = L g R of the reference in NumPy fp64 (mmdft.py:173-174)."""
    pupil = np.asarray(pupil, dtype=np.complex128)
    n = pupil.shape[0]
    left = kernel(n, m, float(pad))
    right = np.exp(-2j * np.pi * np.outer(np.arange(n) - n // 2, np.arange(m) - m // 2)
                   / float(pad)).astype(np.complex128)
    return left @ (pupil @ right)


def count(pupil):
    return int(np.sum(np.abs(np.asarray(pupil)) > 0))


def direct(pupil, pad, m):
    """The reference's PSF formula in NumPy fp64 (mmdft.py:173-177, 201)."""
    field = direct_field(pupil, pad, m)
    psf = field * np.conj(field)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.real(psf) * 100 / np.float64(count(pupil) ** 2)


def field_bound(n, sum_abs):
    """B: |G_dev - G_exact| of every pixel."""
    return (2 * n + 2 * TABLE_ULP + 2) * EPS * float(sum_abs)


def psf_bound(n, sum_abs, field_exact, c):
    """|psf_dev - psf_exact| per pixel."""
    b = field_bound(n, sum_abs)
    return (2 * np.abs(field_exact) * b + b * b) * 100 / float(c) ** 2


def reference_tolerance(pupil, psf_ref):
    """Per pixel: |psf_dev - psf of the reference| on a case of mmdft.npz (|G| from the
    recorded PSF itself: it only scales the bound)."""
    pupil = np.asarray(pupil)
    c = count(pupil)
    field = np.sqrt(np.asarray(psf_ref) / 100) * c
    return psf_bound(pupil.shape[0], np.abs(pupil).sum(), field, c) \
        + 2 * REFERENCE_ERROR * float(np.max(psf_ref))


def random_pupil(n, seed, batch=None):
    """Seeded complex pupil on the unit disc's grid: amplitudes in [0.5, 1], any phase, zero
    outside the disc (for n = 1 the single cell)."""
    rng = np.random.default_rng(seed)
    shape = (n, n) if batch is None else (batch, n, n)
    g = (0.5 + 0.5 * rng.random(shape)) * np.exp(2j * np.pi * rng.random(shape))
    x = np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1)
    xg, yg = np.meshgrid(x, x)
    return np.where(xg ** 2 + yg ** 2 <= 1, g, 0).astype(np.complex128)
