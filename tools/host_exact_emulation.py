#!/usr/bin/env python
"""Host restatements of two kernels' arithmetic against the exact fixtures (CPU only, NumPy):
the figures the comments in csrc/zernike_fit.hip, csrc/huygens.hip, DESIGN.md and profiles/ quote
where they speak of what ONE OTHER choice of arithmetic would give.

    python tools/host_exact_emulation.py [fit] [huygens]

fit      scaled normal equations, Cholesky, and no / one / two refinement steps with the fp64
         residual, on `zernike.basis_numpy` (NumPy sums, no fma: the device's Gram sums are fused
         and come out better in the threshold window), against tests/golden/exact_zernike.npz.
huygens  the Huygens-Fresnel term with error-free products and sums (Dekker, Knuth): R with its
         residual and 1 / lambda as hi + lo, and P - Q either ONE rounded difference (the kernel
         before it carried the low part) or hi + lo (the kernel now), against
         tests/golden/exact_huygens.npz, as a multiple of the bound of tests/_exact.py.
"""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from optiland_amd import zernike as Z  # noqa: E402
from tests import _exact as E  # noqa: E402
from tests import _huygens as H  # noqa: E402
from tests import _zernike_fit as M  # noqa: E402


# ------------------------------------------------------------------ the fit
def fit_errors(g, case, steps=2):
    """[max |c - exact| after 0 ... `steps` refinement steps], bound."""
    x, y, z, kind, k, inten = E.fit_inputs(g, case)
    if inten is not None:
        x, y, z = x[inten > 0], y[inten > 0], z[inten > 0]
    A = Z.basis_numpy(kind, k, x, y)
    G = A.T @ A
    d = 1.0 / np.sqrt(np.diag(G))
    L = np.linalg.cholesky(G * d[:, None] * d[None, :])

    def solve(b):
        return d * np.linalg.solve(L.T, np.linalg.solve(L, d * b))

    want = g[f"{case}/coeffs"]
    c = solve(A.T @ z)
    errs = [float(np.abs(c - want).max())]
    for _ in range(steps):
        c = c + solve(A.T @ (z - A @ c))
        errs.append(float(np.abs(c - want).max()))
    return errs, M.fit_bound(0.0, g[f"{case}/cond"], k, np.abs(want).max())


def fit():
    g = E.load("zernike")
    print("case                         cond      pivot     bound     err0      err1      err2      "
          "lstsq")
    for case in E.names(g, "ladder") + E.names(g, "masked") + E.names(g, "window"):
        errs, bound = fit_errors(g, case)
        pivot = float(g[f"{case}/min_pivot"])
        print(f"{case[4:]:27s} {float(g[case + '/cond']):9.3e} {pivot:9.2e} {bound:9.2e} "
              f"{errs[0]:9.2e} {errs[1]:9.2e} {errs[2]:9.2e} {float(g[case + '/numpy_err']):9.2e}"
              + ("  (pivot <= 1e-8)" if pivot <= 1e-8 else ""))


# ------------------------------------------------------------------ Huygens
def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_diff(a, b):
    s = a - b
    bb = s - a
    return s, (a - (s - bb)) - (b + bb)


def huygens_field(ix, iy, iz, px, py, pz, amp, opd, wl, rp, low_differences=True):
    wl, rp = float(wl), float(rp)
    inv = 1.0 / wl
    _, e = two_prod(wl, inv)
    inv_lo = -((wl * inv - 1.0) + e) / wl
    to = -opd * inv
    w = amp * np.exp(2j * np.pi * (to - np.rint(to)))
    dx, dxl = two_diff(ix[:, None], px[None, :])
    dy, dyl = two_diff(iy[:, None], py[None, :])
    dz, dzl = two_diff(iz[:, None], pz[None, :])
    sx, ex = two_prod(dx, dx)
    sy, ey = two_prod(dy, dy)
    sz, ez = two_prod(dz, dz)
    r2, e1 = two_sum(sz, sy)
    r2, e2 = two_sum(r2, sx)
    r2l = ex + ey + ez + (e1 + e2)
    if low_differences:
        r2l = r2l + 2 * dx * dxl + 2 * dy * dyl + 2 * dz * dzl
    R = np.sqrt(r2)
    p, e = two_prod(R, R)
    d = (r2 - p) - e + r2l
    h = 0.5 / R
    t, te = two_prod(R, inv)
    phase = (t - np.rint(t)) + (te + (R * inv_lo + (d * h) * inv))
    q = 0.5 * (2 * h) * ((dx * px / rp + dy * py / rp + dz * pz / rp) * (2 * h) + 1.0)
    return (w[None, :] * np.exp(2j * np.pi * phase) * q).sum(axis=1)


def huygens():
    g = E.load("huygens")
    print("max |restatement - exact| / bound       P - Q rounded    P - Q as hi + lo")
    for case in E.names(g, "cases"):
        args = tuple(g[f"{case}/{a}"] for a in H.ARGS)
        bound = E.huygens_bound(args[3].size, g[f"{case}/scale"])
        ratios = [float((np.abs(huygens_field(*args, low_differences=low) - g[f"{case}/field"])
                         / bound).max()) for low in (False, True)]
        print(f"{case:38s} {ratios[0]:14.2f} {ratios[1]:19.4f}")


if __name__ == "__main__":
    for name in sys.argv[1:] or ["fit", "huygens"]:
        {"fit": fit, "huygens": huygens}[name]()
