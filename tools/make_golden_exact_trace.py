#!/usr/bin/env python
"""Writes tests/golden/exact_trace.npz: per case (tests/_exact_trace.py: CASES) and dtype the
inputs rounded to that dtype, their trace at 50 digits rounded to float64 once, the mask of the
rays the tests look at, and per row and group (position, direction, path, intensity) the error of
the same plain trace at the dtype's own precision (the yardstick), the scale and -- fp64 -- the
error of the oracle, the C restatement of the reference's formulae.  Needs mpmath.

    python tools/make_golden_exact_trace.py [--jobs N] [case ...]
"""

from __future__ import annotations

import argparse
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _exact_trace as X  # noqa: E402

DPS = 50


def make(name, tag, only=None):
    """The arrays of one case and dtype; with `only` (ray indices) just the inputs and the truth
    of those rays (the other columns NaN)."""
    import mpmath
    from mpmath import mp

    mp.dps = DPS
    table = X.case_table(name, tag)
    inputs = np.ascontiguousarray(X.case_rays(name).astype(X.NP_DTYPE[tag]))
    truth, keep, kappa = X.trace_bundle(mp, table, inputs, want_kappa=only is None, only=only)
    # (row 0, the object row, records the inputs as they are: not stored a second time)
    out = {f"{name}/{tag}/in": inputs, f"{name}/{tag}/truth": truth[1:]}
    if only is not None:
        return out
    yard, _, _ = X.trace_bundle(mp, table, inputs, prec=X.PREC[tag])
    keep &= np.isfinite(yard).all(axis=(0, 1))
    n = keep.size
    assert n - int(keep.sum()) <= X.MAX_DROPPED * n, (name, tag, n - int(keep.sum()), n)
    out[f"{name}/{tag}/keep"] = keep
    out[f"{name}/{tag}/kappa"] = kappa
    out[f"{name}/{tag}/scale"] = X.scales(truth, keep, table)
    out[f"{name}/{tag}/znorm"] = X.conic_normal_terms(table, truth, keep)
    out[f"{name}/{tag}/yard"] = X.group_max(yard - truth, keep)
    if tag == "f64":
        from oracle import oracle
        rays = {k: inputs[j].astype(np.float64) for j, k in
                enumerate(("x", "y", "z", "L", "M", "N", "i"))}
        ref = oracle.trace(table, rays, 0, record=True)["record"]
        out[f"{name}/{tag}/ref"] = X.group_max(ref - truth, keep)
    assert mpmath.mp.dps == DPS
    return out


def _job(args):
    return make(*args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("cases", nargs="*", default=list(X.CASES))
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=X.GOLD)
    args = ap.parse_args()
    from oracle import oracle
    oracle.build(force=False)
    jobs = [(c, t) for c in args.cases for t in X.TAGS]
    made = {}
    with multiprocessing.Pool(args.jobs) as pool:
        for (case, tag), part in zip(jobs, pool.imap(_job, jobs)):
            made.update(part)
            keep = part[f"{case}/{tag}/keep"]
            print(f"{case:24s} {tag}: kept {int(keep.sum())}/{keep.size}  yard pos/dir "
                  f"{part[f'{case}/{tag}/yard'][-1, 0]:.2e} / {part[f'{case}/{tag}/yard'][-1, 1]:.2e}",
                  flush=True)
    if set(args.cases) != set(X.CASES) and os.path.exists(args.out):
        made = {**dict(np.load(args.out)), **made}
    np.savez_compressed(args.out, **made)
    print(f"{args.out}: {os.path.getsize(args.out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
