"""Shared pieces of the tests against exact references: the fixtures of
tools/make_golden_exact.py (mpmath at 50 digits, rounded to fp64 once) and the bounds the
kernels are held to against them.  The GPU tests read the fixtures only; mpmath is needed by
the generator and by tests/test_exact_fixtures_cpu.py alone.

Every bound is rounding analysis of the kernel's own operation count; none is a measured figure:
  eval     (2 s + 2 + K) 2^-52 sum_j |c_j| |Z|_j -- ONE Horner evaluation of every radial
           polynomial (gamma_(2s+2), s = ZK_MAX_RADIAL; the truth does not round) and a K-term
           sum, |Z|_j = `_zernike_fit.abs_basis`;
  sampled  n 2^-52 for the normalised n-term sum, plus 2 pi times the phase error in cycles:
           2^-52 max|opd| for the one rounded difference opd - W and the eval bound of W;
  Huygens  (n_pupil + 32) 2^-52 sum_j |a_j q_mj / R_mj| per pixel: the n_pupil-term sum and
           32 ulp for everything inside a term."""

from __future__ import annotations

import os

import numpy as np

from optiland_amd import _capi
from tests import _zernike_fit as M
from tests._util import GOLDEN

EPS = M.EPS


def load(name):
    """tests/golden/exact_<name>.npz as a dict."""
    return dict(np.load(os.path.join(GOLDEN, f"exact_{name}.npz")))


def names(g, key):
    return [str(c) for c in np.atleast_1d(g[key])]


def fit_inputs(g, case):
    """(x, y, z, kind, K, intensity or None) of a conditioning case."""
    return (g[f"{case}/x"], g[f"{case}/y"], g[f"{case}/z"], str(g[f"{case}/kind"]),
            int(g[f"{case}/num_terms"]), g.get(f"{case}/intensity"))


def eval_limit(num_terms):
    return (2 * _capi.ZK_MAX_RADIAL + 2 + num_terms) * EPS


# `abs_basis` reads `zernike.term_table`, the table under test: a wrong radial coefficient there
# would move these bounds with the kernel.  test_eval_against_the_exact_basis holds it to the
# fixture's `abs_basis` (mpmath, the factorial formula) at K = 120, which covers every term.
def eval_bound(kind, coeffs, x, y):
    """Per point: |device - exact| of sum_j c_j Z_j."""
    c = np.asarray(coeffs, dtype=np.float64)
    return eval_limit(c.size) * (M.abs_basis(kind, c.size, x, y) @ np.abs(c))


def smtf_bound(kind, coeffs, x, y, opd, shifts):
    """|device - exact| of every frequency of one sampled-MTF call."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    waves = 0.0
    for dx, dy in np.asarray(shifts, dtype=np.float64).reshape(-1, 2):
        xs, ys = x - dx, y - dy
        inside = ~(np.sqrt(xs ** 2 + ys ** 2) > 1.0)
        if inside.any():
            waves = max(waves, float(eval_bound(kind, coeffs, xs[inside], ys[inside]).max()))
    return float(x.size * EPS + 2 * np.pi * (EPS * np.abs(opd).max() + waves))


def huygens_bound(n_pupil, scale):
    return (n_pupil + 32) * EPS * np.asarray(scale)
