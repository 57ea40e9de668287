"""Shared pieces of the geometric MTF tests: the golden fixture (tools/make_golden_mtf.py) and a
NumPy fp64 restatement of the reference's `GeometricMTF._compute_field_data`
(mtf/geometric.py:179-204) with the loop over the frequencies written as one outer product --
the yardstick of `ol_geometric_mtf`."""

from __future__ import annotations

import os

import numpy as np

from tests._util import GOLDEN

SYSTEMS = {"cooke": "cooke_generic", "dgauss": "double_gauss"}


def golden():
    return dict(np.load(os.path.join(GOLDEN, "geometric_mtf.npz")))


def cases(g=None):
    g = golden() if g is None else g
    return [str(c) for c in g["cases"]]


def fft_cases(g=None):
    g = golden() if g is None else g
    return [str(c) for c in g["fft_cases"]]


def n_fields(g, case):
    return int(g[f"{case}/fields"].shape[0])


def hits(g, case):
    """[(x, y) per field] of a case (stored once per lens / num_rays / distribution)."""
    owner = str(g[f"{case}/hits_of"])
    return [(g[f"{owner}/x{k}"], g[f"{owner}/y{k}"]) for k in range(n_fields(g, case))]


def curves(g, case):
    """The case's curves in kernel order: [tangential (y), sagittal (x)] per field."""
    return [c for x, y in hits(g, case) for c in (y, x)]


def kwargs(g, case):
    """Constructor keywords of a case (for the reference's and the stand-alone class)."""
    mf = float(g[f"{case}/max_freq_in"])
    return dict(num_rays=int(g[f"{case}/num_rays"]), distribution=str(g[f"{case}/distribution"]),
                num_points=int(g[f"{case}/num_points"]), scale=bool(g[f"{case}/scale"]),
                max_freq="cutoff" if np.isnan(mf) else mf)


def scale_of(g, case):
    """The per-frequency factor handed to the kernel: diff_limited_mtf, or None for scale=False
    (the reference then stores the scalar 1)."""
    return g[f"{case}/diff_limited_mtf"] if bool(g[f"{case}/scale"]) else None


def direct_mtf(x, freq, scale=None, n_bins=None):
    """(mtf, counts, edges) of one curve, as mtf/geometric.py:193-204 computes them."""
    freq = np.asarray(freq, dtype=np.float64)
    n_bins = freq.size + 1 if n_bins is None else n_bins
    A, edges = np.histogram(np.asarray(x, dtype=np.float64), bins=n_bins)
    xc = (edges[1:] + edges[:-1]) / 2
    dx = xc[1] - xc[0] if n_bins > 1 else 1.0
    arg = 2 * np.pi * freq[:, None] * xc[None, :]
    den = np.sum(A * dx)
    Ac = np.sum(A * np.cos(arg) * dx, axis=1) / den
    As = np.sum(A * np.sin(arg) * dx, axis=1) / den
    mtf = np.sqrt(Ac ** 2 + As ** 2)
    return (mtf if scale is None else mtf * scale), A, edges


def numpy_geometric_mtf(curves_, freq, scale=None, n_bins=None):
    """Stand-in for `engine.geometric_mtf` on the host: (curves, num_points) float64."""
    return np.array([direct_mtf(np.asarray(c), freq, scale, n_bins)[0] for c in curves_])
