"""Zernike polynomials on the device, stand-alone (no reference package needed).

The host side of `csrc/zernike_fit.hip`: the (n, m) index tables of the three numbering schemes
the reference knows (zernike/fringe.py, standard.py, noll.py), the normalisation constants, the
exact radial coefficients, and the term table the kernels read.  `ZernikeFit` mirrors the
reference's class of that name (zernike/fit.py:33-118): `.coeffs`, `.poly(x, y)`, the index tables.

Numbering (Niu & Tian, J. Opt. 24 (2022) 123001, section 2; Noll, J. Opt. Soc. Am. 66 (1976) 207):
  fringe    1-based, number = (1 + (n + |m|) / 2)^2 - 2 |m| + (1 if m < 0 else 0); norm 1
  standard  OSA / ANSI, 0-based, number = (n (n + 2) + m) / 2;    norm sqrt((2 n + 2) / (1 + [m = 0]))
  noll      1-based, number = n (n + 1) / 2 + |m| + c with c = 0 for (m > 0, n mod 4 <= 1) and
            (m < 0, n mod 4 >= 2), else 1;                        norm as standard
"""

from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

from . import _capi

KINDS = ("fringe", "standard", "noll")
ZK_MAX_TERMS = _capi.ZK_MAX_TERMS


def _number(kind: str, n: int, m: int) -> int:
    """The position of (n, m) in the scheme's own numbering (n - m even)."""
    a = abs(m)
    if kind == "fringe":
        return (1 + (n + a) // 2) ** 2 - 2 * a + (1 if m < 0 else 0)
    if kind == "standard":
        return (n * (n + 2) + m) // 2
    if kind == "noll":
        low = n % 4 <= 1
        c = 0 if (m > 0 and low) or (m < 0 and not low) else 1
        return n * (n + 1) // 2 + a + c
    raise ValueError(f"Invalid Zernike type '{kind}'. Choose from: {list(KINDS)}")


def check_terms(kind: str, num_terms, who: str = "zernike") -> int:
    if kind not in KINDS:
        raise ValueError(f"Invalid Zernike type '{kind}'. Choose from: {list(KINDS)}")
    if isinstance(num_terms, bool) or int(num_terms) != num_terms:
        raise ValueError(f"{who}: num_terms must be an integer, got {num_terms!r}")
    num_terms = int(num_terms)
    if not 1 <= num_terms <= ZK_MAX_TERMS:
        raise ValueError(f"{who}: num_terms {num_terms} is outside 1..{ZK_MAX_TERMS} "
                         "(ZK_MAX_TERMS)")
    return num_terms


@lru_cache(maxsize=None)
def _indices(kind: str, num_terms: int):
    # every (n, m) up to a radial order that certainly holds the first `num_terms` numbers: the
    # fringe scheme orders by (n + |m|) / 2, whose level s ends at number (s + 1)^2; the other
    # two order by n, whose level ends at (n + 1) (n + 2) / 2 terms
    if kind == "fringe":
        top = 2 * math.isqrt(num_terms - 1) + 2
    else:
        top = 0
        while (top + 1) * (top + 2) // 2 < num_terms:
            top += 1
    found = sorted((_number(kind, n, m), n, m) for n in range(top + 1)
                   for m in range(-n, n + 1, 2))
    return tuple((n, m) for _, n, m in found[:num_terms])


def indices(kind: str, num_terms: int):
    """((n, m), ...) of the first `num_terms` terms of a scheme, in the scheme's order."""
    return _indices(kind, check_terms(kind, num_terms))


def norm_constant(kind: str, n: int, m: int) -> float:
    if kind == "fringe":
        return 1.0
    return math.sqrt((2 * n + 2) / (2 if m == 0 else 1))


def radial_coefficients(n: int, m: int):
    """c_k, k = 0 ... (n - |m|) / 2: the coefficient of r^(n - 2k) in R_n^|m| (exact integers)."""
    a = abs(m)
    f = math.factorial
    return [(-1) ** k * f(n - k) // (f(k) * f((n + a) // 2 - k) * f((n - a) // 2 - k))
            for k in range((n - a) // 2 + 1)]


@lru_cache(maxsize=None)
def _term_table(kind: str, num_terms: int):
    idx = _indices(kind, num_terms)
    stride = 1 + _capi.ZK_MAX_RADIAL
    ti = np.zeros((num_terms, 4), dtype=np.int32)
    tf = np.zeros((num_terms, stride), dtype=np.float64)
    order = sorted(range(num_terms), key=lambda j: (abs(idx[j][1]), j))   # grouped by |m|
    for row, j in enumerate(order):
        n, m = idx[j]
        c = radial_coefficients(n, m)
        if len(c) > _capi.ZK_MAX_RADIAL or abs(m) > _capi.ZK_MAX_M or \
                any(abs(v) >= 2 ** 53 for v in c):
            raise ValueError(f"zernike term (n, m) = ({n}, {m}) does not fit the kernel's table")
        ti[row] = (j, n, m, len(c))
        tf[row, 0] = norm_constant(kind, n, m)
        tf[row, 1:1 + len(c)] = c
    ti.setflags(write=False)
    tf.setflags(write=False)
    return ti, tf


def term_table(kind: str, num_terms: int):
    """(term_i (K, 4) int32, term_f (K, 1 + ZK_MAX_RADIAL) float64): the table of
    include/optiland_hip.h, rows grouped by ascending |m| (read-only arrays, cached)."""
    return _term_table(kind, check_terms(kind, num_terms))


def basis_numpy(kind: str, num_terms: int, x, y) -> np.ndarray:
    """(points, K) design matrix on the host, the kernels' arithmetic restated in NumPy (used by
    the CPU tests as the stand-in for the kernels, and nowhere on a hot path)."""
    ti, tf = term_table(kind, num_terms)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    r2 = x * x + y * y
    r = np.sqrt(r2)
    ok = r > 0
    c1 = np.where(ok, x / np.where(ok, r, 1.0), 1.0)
    s1 = np.where(ok, y / np.where(ok, r, 1.0), 0.0)
    cm, sm, rp, mm = np.ones_like(r), np.zeros_like(r), np.ones_like(r), 0
    A = np.empty((x.size, num_terms))
    for (col, _n, m, nc), f in zip(ti, tf):
        while mm < abs(m):
            cm, sm = cm * c1 - sm * s1, sm * c1 + cm * s1
            rp = rp * r
            mm += 1
        v = np.full_like(r, f[1])
        for k in range(1, nc):
            v = v * r2 + f[1 + k]
        A[:, col] = f[0] * (v * rp) * (cm if m >= 0 else sm)
    return A


class ZernikeFit:
    """Least-squares Zernike fit of z over the points (x, y) on the device (zernike/fit.py:33-118
    with `ol_zernike_fit`).  `coeffs`: (num_terms,) float64 device tensor; `poly(x, y)`: the
    fitted sum at Cartesian points (`ol_zernike_eval`); `indices`: the scheme's (n, m) table;
    `status`: the kernel's status word (0).  A rank-deficient or non-finite problem raises
    ValueError: the reference answers those with `lstsq`'s minimum-norm solution, which normal
    equations cannot give."""

    def __init__(self, x, y, z, zernike_type: str = "fringe", num_terms: int = 36, *,
                 intensity=None, device=None):
        self.num_terms = check_terms(zernike_type, num_terms, "ZernikeFit")
        self.zernike_type = zernike_type
        self.indices = indices(zernike_type, self.num_terms)
        self.x, self.y, self.z, self.intensity = x, y, z, intensity
        self.device = device
        self.coeffs, self.status = self._fit()
        if self.status:
            raise ValueError(f"ZernikeFit: {status_text(self.status)}")
        self.num_pts = int(np.prod(tuple(getattr(x, "shape", np.shape(x)))))

    def _fit(self):
        from .engine import zernike_fit
        c, status = zernike_fit(self.x, self.y, self.z, self.zernike_type, self.num_terms,
                                intensity=self.intensity, device=self.device)
        return c, int(status)

    def poly(self, x, y):
        from .engine import zernike_eval
        return zernike_eval(self.coeffs, self.zernike_type, x, y, device=self.device)

    def residual_rms(self):
        """sqrt(mean((poly - z)^2)) over the fitted points (fit.py:210-213)."""
        d = self.poly(self.x, self.y) - self.z
        return (d * d).mean() ** 0.5


def status_text(status: int) -> str:
    why = []
    if status & _capi.ZK_TOO_FEW:
        why.append("fewer valid points than terms")
    if status & _capi.ZK_RANK_DEFICIENT:
        why.append("the design matrix is rank deficient (or too ill-conditioned for normal "
                   "equations)")
    if status & _capi.ZK_NONFINITE:
        why.append("a non-finite input")
    return "; ".join(why) or "ok"
