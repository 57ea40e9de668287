#!/usr/bin/env python
"""tests/golden/exact_mmdft.npz: the matrix-multiply DFT of the MMDFT PSF (psf/mmdft.py:157-283)
evaluated with mpmath at 50 digits from fp64 inputs and rounded to fp64 once, for
tests/test_gpu_mmdft_exact.py and the fixture self-check of tests/test_mmdft_cpu.py.

    W[v][j] = exp(-2 pi i (v - M/2) (j - N/2) / pad)   (pad: the fp64 value, exactly)
    G = W g W^T,   psf = |G|^2 100 / c^2,   c = #{|g| > 0}

in the two-stage form T = g W^T, G = W T (N^2 M + N M^2 products per case), on seeded random
complex pupils (tests/_mmdft.random_pupil).  Each case also holds the result of the reference's
own formula in NumPy fp64 on the same inputs (tests/_mmdft.direct) and sum |g|.

It PRINTS the reference error -- the largest |psf_numpy - psf_exact| / max(psf_exact) over the
cases -- which tests/_mmdft.py holds as REFERENCE_ERROR: the reference's own distance from the
exact transform, measured here on the CPU, no device involved.

Fixed seeds; the .npz members are written uncompressed with a constant time stamp, so a rerun
reproduces the file byte for byte.

    python tools/make_golden_exact_mmdft.py      (CPU only, needs mpmath)
"""

from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.dont_write_bytecode = True
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402

from tests import _mmdft as MM  # noqa: E402
from tools.make_golden_exact import save  # noqa: E402

mp.mp.dps = 50
GOLD = os.path.join(ROOT, "tests", "golden", "exact_mmdft.npz")
# (N, M, pad): one cell; M < N and a non-integer pad; the reference's defaults at 33 / 48; the
# golden double-Gauss geometry (odd N, non-integer pad); M < N at a full tile
CASES = [(1, 1, 1.0), (17, 7, 23.5), (33, 48, 48.0), (45, 105, 105.65036602741444),
         (64, 33, 70.25)]


def name_of(n, m):
    return f"n{n}_m{m}"


def exact(pupil, pad, m):
    """(G, psf) as lists of rows of mpc / mpf."""
    n = pupil.shape[0]
    padx = mp.mpf(float(pad))
    w = [[mp.expjpi(-2 * mp.mpf((v - m // 2) * (j - n // 2)) / padx) for j in range(n)]
         for v in range(m)]
    g = [[mp.mpc(float(z.real), float(z.imag)) for z in row] for row in pupil]
    t = [[mp.fsum(g[y][x] * w[u][x] for x in range(n)) for u in range(m)] for y in range(n)]
    field = [[mp.fsum(w[v][y] * t[y][u] for y in range(n)) for u in range(m)] for v in range(m)]
    c = MM.count(pupil)
    psf = [[(z.real ** 2 + z.imag ** 2) * 100 / mp.mpf(c) ** 2 for z in row] for row in field]
    return field, psf


def main():
    out = {"cases": np.array([name_of(n, m) for n, m, _ in CASES])}
    worst = (0.0, "")
    for k, (n, m, pad) in enumerate(CASES):
        name = name_of(n, m)
        pupil = MM.random_pupil(n, seed=20250 + k)
        field, psf = exact(pupil, pad, m)
        field = np.array([[complex(float(z.real), float(z.imag)) for z in row] for row in field])
        psf = np.array([[float(p) for p in row] for row in psf])
        np_field, np_psf = MM.direct_field(pupil, pad, m), MM.direct(pupil, pad, m)
        sum_abs, c = float(np.abs(pupil).sum()), MM.count(pupil)
        err_f = float(np.max(np.abs(np_field - field)))
        err_p = float(np.max(np.abs(np_psf - psf)) / np.max(psf))
        out[f"{name}/pupil"] = pupil
        out[f"{name}/pad_size"] = np.float64(pad)
        out[f"{name}/image_size"] = np.int64(m)
        out[f"{name}/field"] = field
        out[f"{name}/psf"] = psf
        out[f"{name}/numpy_psf"] = np_psf
        out[f"{name}/numpy_field_err"] = np.float64(err_f)
        out[f"{name}/sum_abs"] = np.float64(sum_abs)
        out[f"{name}/count"] = np.int64(c)
        bound = MM.field_bound(n, sum_abs)
        print(f"{name:10s} pad {pad:<20.17g} c {c:5d} sum|g| {sum_abs:9.3f}  NumPy formula: "
              f"field {err_f:.3e} ({err_f / bound:.2f} x the kernel's bound B), psf {err_p:.3e} "
              f"of the peak")
        if err_p > worst[0]:
            worst = (err_p, name)
    print(f"reference error: {worst[0]:.3e} of the peak (case {worst[1]})")
    save(GOLD, out)
    print(f"{GOLD}: {os.path.getsize(GOLD)} bytes")


if __name__ == "__main__":
    main()
