#!/usr/bin/env python
"""Writes tests/golden/exact_front.npz from the definitions of tests/_exact_front.py: generated
rays, the generating trace, spot moments, chief-ray references and OPD of every case at 50 digits
(rounded to float64 once), the errors of the same plain formulae at 53 and 24 bits (the
yardsticks), the scales and the masks.  Numbers only.  Needs mpmath.

    python tools/make_golden_exact_front.py [--jobs N]
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

from tests import _exact_front as F  # noqa: E402
from tests import _exact_trace as X  # noqa: E402

DPS = 50
NAN8 = (float("nan"),) * 8


def _fl(v):
    return [float(a) for a in v]


def _err(mp, got, want):
    """max |got - want| of two sequences of mpf (None: skipped), formed at 50 digits."""
    worst = 0.0
    for a, b in zip(got, want):
        if a is not None and b is not None:
            worst = max(worst, float(abs(a - b)))
    return worst


def apod_numpy(rg, px, py):
    """The reference's own NumPy lines (apodization/*.py) on arrays of the dtype of px."""
    kind, a, b = int(rg.get("apod_kind", 0)), rg.get("apod_a", 0.0), rg.get("apod_b", 0.0)
    if kind == 0:
        return np.ones_like(px)
    if kind == 1:
        return np.exp(-(px**2 + py**2) / (2 * a**2))
    r = (px**2 + py**2) ** 0.5
    if kind == 2:
        return np.where(r < a, np.cos((np.pi * r) / (2 * a)) ** 2, 0.0).astype(px.dtype)
    if kind == 3:
        return np.where(r < a / 2, 0.5 * (1 - np.cos((2 * np.pi * r) / a)), 0.0).astype(px.dtype)
    if kind == 4:
        with np.errstate(invalid="ignore"):
            return np.where(r < a, (1 - (r / a) ** 2) ** b, 0.0).astype(px.dtype)
    if kind == 5:
        return np.exp(-((r / a) ** b))
    flat = a * (1 - b / 2)
    taper = 0.5 * (1 + np.cos(np.pi * (r - flat) / (a * b / 2)))
    out = np.where(r <= flat, 1.0, 0.0)
    return np.where((r > flat) & (r < a), taper, out).astype(px.dtype)


# ---------------------------------------------------------------------------------------------
def make_gen(name, only=None):
    """The generated rays of one case: every subcase's truth and per dtype the yardstick."""
    from mpmath import mp
    mp.dps = DPS
    rg = F.table_for(name).raygen
    px, py = F.gen_pupil(name)
    n = px.size
    out = {f"gen/{name}/pxy": np.stack([px, py]).astype(np.float32)}
    for sub, (field, vig, flags) in enumerate(F.GEN_CASES[name]):
        key = f"gen/{name}/{sub}"
        idx = range(n) if only is None else only
        rays = {j: gen_ray_at(mp, None, rg, field, vig, flags, px[j], py[j]) for j in idx}
        truth = np.full((7, n), np.nan)
        for j, r in rays.items():
            truth[:, j] = _fl(r)
        out[f"{key}/truth"] = truth
        out[f"{key}/par"] = np.array([*field, *vig, flags], dtype=np.float64)
        if only is not None:
            continue
        # no pupil point within rounding of a radius where the apodisation changes branch
        spx, spy = (px * vig[0], py * vig[1]) if flags & F.PRESCALE else (px, py)
        assert all(np.abs(np.hypot(spx, spy) - e).min() > 1e-3 for e in F.apod_edges(rg)), name
        out[f"{key}/scale"] = np.array([np.abs(truth[:3]).max(), 1.0, 1.0])
        for tag in F.TAGS:
            yard = {j: gen_ray_at(mp, F.PREC[tag], rg, field, vig, flags, px[j], py[j])
                    for j in idx}
            e = [max(_err(mp, [yard[j][p] for j in idx], [rays[j][p] for j in idx])
                     for p in grp) for grp in ((0, 1, 2), (3, 4, 5), (6,))]
            out[f"{key}/{tag}/yard"] = np.array(e)
            dt = X.NP_DTYPE[tag]
            got = apod_numpy(rg, spx.astype(dt), spy.astype(dt)).astype(np.float64)
            out[f"{key}/{tag}/enumpy"] = np.array(
                max(float(abs(mp.mpf(float(got[j])) - rays[j][6])) for j in idx))
    if name == "cooke_generic" and only is None:
        # one out-of-range point per flag: the status word of every combination of the checks
        ppx, ppy, phx, phy = f32_list([0.0, 1.5, 0.0]), f32_list([0.0, 0.0, 0.0]), \
            f32_list([0.0, 0.0, 1.25]), f32_list([0.0, 0.0, 0.0])
        rows = []
        for flags in (0, F._capi.RAYGEN_CHECK_PUPIL, F._capi.RAYGEN_CHECK_FIELD, F.CHECKS):
            st = 0
            for a, b, c, d in zip(phx, phy, ppx, ppy):
                st |= F.gen_ray(mp, rg, a, b, c, d, 1.0, 1.0, flags)[1]
            rows.append([flags, st])
        out[f"gen/{name}/probe_in"] = np.array([ppx, ppy, phx, phy], dtype=np.float32)
        out[f"gen/{name}/probe"] = np.array(rows, dtype=np.int64)
    assert mp.dps == DPS
    return out


def f32_list(v):
    return [float(a) for a in F.f32(v)]


def gen_ray_at(mp, prec, rg, field, vig, flags, px, py):
    old = mp.prec
    if prec is not None:
        mp.prec = prec
    try:
        return F.gen_ray(mp, rg, field[0], field[1], px, py, vig[0], vig[1], flags)[0]
    finally:
        mp.prec = old


# ---------------------------------------------------------------------------------------------
def _bundle(mp, table, prec, px, py, hx, hy, vig, idx, want_kappa=False):
    """Generate and trace the rays `idx` at `prec` bits (None: the precision in force).
    Returns (rows per ray: list of 8-tuples of mpf or None, info per ray)."""
    old = mp.prec
    if prec is not None:
        mp.prec = prec
    try:
        rows, infos = {}, {}
        for j in idx:
            ray, _ = F.gen_ray(mp, table.raygen, hx[j], hy[j], px[j], py[j], vig[0], vig[1], 0)
            rows[j], infos[j] = X.trace_ray(mp, table, list(ray) + [mp.mpf(0)],
                                            want_kappa=want_kappa)
        return rows, infos
    finally:
        mp.prec = old


def _record(rows, n, nrows):
    rec = np.full((nrows, 8, n), np.nan)
    for j, got in rows.items():
        for k, row in enumerate(got):
            if row is not None:
                rec[k, :, j] = _fl(row)
    return rec


def make_trace(name, only=None):
    """One spot / trace / chief / OPD table: every array of the fixture under trace/, spot/,
    chief/ and opd/ of that name; with `only` (ray indices) just the truth of those rays."""
    from mpmath import mp
    mp.dps = DPS
    table = F.table_for(name, "f64")
    nrows = table.num_surfaces
    px, py, hx, hy = F.trace_inputs(name)
    off, vig = F.TRACE_CASES[name]
    n, half = px.size, px.size // 2
    idx = range(n) if only is None else only
    rows, infos = _bundle(mp, table, None, px, py, hx, hy, vig, idx, want_kappa=only is None)
    truth = _record(rows, n, nrows)
    out = {f"trace/{name}/in": np.stack([px, py, hx, hy]).astype(np.float32),
           f"trace/{name}/vig": np.array(vig),
           f"trace/{name}/rows": truth[:, :, half:],          # every row of the off-axis bundle
           f"trace/{name}/image": truth[-1]}                  # the image row of both
    if only is not None:
        return out
    lost = np.array([infos[j]["lost"] for j in idx])
    clipped = np.array([infos[j]["clipped"] for j in idx])
    keep = np.array([not (i["lost"] or i["clipped"] or i["min_cos"] < X.MIN_COS
                          or i["min_snell"] < X.MIN_SNELL) for i in infos.values()])
    # the conditions of the sums: no ray is lost, and whatever is not clipped is kept
    assert not lost.any() and np.array_equal(keep, ~clipped), (name, lost.sum(), keep.sum())
    assert int(table.raygen.get("apod_kind", 0)) in (0, 1)    # (the intensity never reaches 0)
    kappa = np.zeros(nrows)
    for j in idx:
        if keep[j]:
            kappa = np.maximum(kappa, infos[j]["kappa"])
    out[f"trace/{name}/keep"] = keep
    out[f"trace/{name}/kappa"] = kappa
    out[f"trace/{name}/scale"] = X.scales(truth, keep, table)
    out[f"trace/{name}/znorm"] = X.conic_normal_terms(table, truth, keep)
    # per row the longest step into it over the cosine of incidence there, and the smallest
    # cosine: what carries a direction deviation into the next hit (`_exact_front.trace_bound`)
    lever, cosmin = np.zeros(nrows), np.ones(nrows)
    for j in idx:
        if keep[j]:
            for k, c in infos[j]["cos"]:
                step = abs(truth[k, 7, j] - truth[k - 1, 7, j]) / float(table.optics[k, 0]["n1"])
                lever[k], cosmin[k] = max(lever[k], step / c), min(cosmin[k], c)
    out[f"trace/{name}/lever"], out[f"trace/{name}/cosmin"] = lever, cosmin
    yrows = {}
    for tag in F.TAGS:
        yrows[tag], yinfo = _bundle(mp, F.table_for(name, tag), F.PREC[tag], px, py, hx, hy, vig,
                                    idx)
        yard = _record(yrows[tag], n, nrows)
        assert np.isfinite(yard[:, :, keep]).all(), (name, tag)
        assert not any(i["lost"] for i in yinfo.values()), (name, tag)
        out[f"trace/{name}/{tag}/yard"] = X.group_max(yard - truth, keep)
    # no truth hit closer to an aperture edge than the fp32 position bound of its row
    fix = dict(out)
    b32 = F.trace_bound(fix, name, "f32")
    margins = np.array([F.edge_margin(table, truth[k, :2], k).min() for k in range(nrows)])
    assert np.all(margins > b32[:, 0]), (name, margins, b32[:, 0])
    out[f"trace/{name}/margin"] = margins
    assert 0 < int(keep.sum()) and n - int(keep.sum()) <= 0.35 * n, (name, keep.sum())
    # ---- spot moments about (0, 0) and about the truth's centroid rounded to the dtype
    img = [rows[j][-1] for j in range(n)]
    xs, ys, ii = [r[0] for r in img], [r[1] for r in img], [r[6] for r in img]
    cnt = int(keep.sum())
    mean = (float(sum(x for x, k in zip(xs, keep) if k) / cnt),
            float(sum(y for y, k in zip(ys, keep) if k) / cnt))
    for tag in F.TAGS:
        dt = X.NP_DTYPE[tag]
        centers = [(0.0, 0.0), (float(dt(mean[0])), float(dt(mean[1])))]
        out[f"spot/{name}/{tag}/center"] = np.array(centers)
        out[f"spot/{name}/{tag}/moments"] = np.array(
            [_fl(F.spot_sums(mp, xs, ys, ii, cx, cy)) for cx, cy in centers])
        assert out[f"spot/{name}/{tag}/moments"][0, 0] == cnt
    # ---- chief-ray references and the OPD against them, per field (fp64 only)
    rg = table.raygen
    yrow = yrows["f64"]
    for f, field in enumerate((F.AXIS, off)):
        w = F.wave_params(table, field)
        sel = list(range(f * half, (f + 1) * half))
        kp = keep[sel]
        j0 = sel[0]
        assert px[j0] == 0 and py[j0] == 0
        chief = F.last_step(mp, rows[j0][-1], table.last_thickness)
        mp.prec = 53
        ychief = F.last_step(mp, yrow[j0][-1], table.last_thickness)
        mp.dps = DPS
        for kind in F.REFS:
            key = f"opd/{name}/{f}/{kind}"
            planar = kind == "plane"
            ref = F.chief_reference(mp, chief, rg["pupil_z"], planar, w["n_image"])
            mp.prec = 53
            yref = F.chief_reference(mp, ychief, rg["pupil_z"], planar, w["n_image"])
            mp.dps = DPS
            names = ("xc", "yc", "zc", "R", "opd_ref", "nx", "ny", "nz")
            out[f"{key}/ref"] = np.array([float(ref[k]) for k in names])
            out[f"{key}/chief"] = np.array(_fl(chief))
            out[f"{key}/ref_yard"] = np.array(
                [_err(mp, [yref[k] for k in g], [ref[k] for k in g])
                 for g in (("xc", "yc", "zc"), ("R",), ("opd_ref",), ("nx", "ny", "nz"))])
            out[f"{key}/chief_yard"] = np.array(
                [_err(mp, [ychief[p] for p in g], [chief[p] for p in g])
                 for g in ((0, 1, 2), (3, 4, 5), (7,), (6,))])
            # (a) the reference as INPUT: the truth's, rounded to fp64
            par = {k: float(w[k]) for k in ("n_image", "wavelength_um", "half_epd", "ux", "uy",
                                            "last_thickness", "last_absorb")}
            par.update({k: float(ref[k]) for k in names})
            out[f"{key}/par"] = np.array([par[k] for k in F.WF_KEYS])
            ref_a = dict(ref, **{k: mp.mpf(float(ref[k])) for k in names})

            def run(reference, source, rounded=False):
                got = []
                for j in sel:
                    ray = F.last_step(mp, source[j][-1], table.last_thickness)
                    if rounded:
                        ray = tuple(+mp.mpf(float(v)) for v in ray)
                    got.append(F.opd_of_ray(mp, reference, w, ray, px[j], py[j]))
                return got

            ta, tb, tc = run(ref_a, rows), run(ref, rows), run(ref_a, rows, rounded=True)
            mp.prec = 53
            ya, yb, yc = run(ref_a, yrow), run(yref, yrow), run(ref_a, rows, rounded=True)
            mp.dps = DPS
            keep_i = [i for i, k in enumerate(kp) if k]
            opd_a = np.array([float(v[0]) for v in ta])
            pup_a = np.array([_fl(v[1]) for v in ta]).T
            out[f"{key}/opd"] = opd_a
            out[f"{key}/pupil"] = pup_a
            for lab, tt in (("b", tb), ("c", tc)):
                out[f"{key}/d_opd_{lab}"] = np.array(
                    [float(v[0] - u[0]) for v, u in zip(tt, ta)], dtype=np.float32)
                out[f"{key}/d_pupil_{lab}"] = np.array(
                    [[float(p - q) for p, q in zip(v[1], u[1])] for v, u in zip(tt, ta)],
                    dtype=np.float32).T
            for lab, tt, yy in (("a", ta, ya), ("b", tb, yb), ("c", tc, yc)):
                out[f"{key}/yard_{lab}"] = np.array([
                    _err(mp, [yy[i][0] for i in keep_i], [tt[i][0] for i in keep_i]),
                    max(_err(mp, [yy[i][1][p] for i in keep_i], [tt[i][1][p] for i in keep_i])
                        for p in range(3))])
            # rays of the stand-alone kernel: the truth's image rays rounded to fp64
            out[f"{key}/rays_c"] = np.array(
                [_fl(F.last_step(mp, rows[j][-1], table.last_thickness)) for j in sel]).T[
                    [0, 1, 2, 3, 4, 5, 7]]
            # scales and the factors that carry a direction / position error into t
            wl = w["wavelength_um"] * 1e-3
            path = max(abs(float(rows[j][-1][7])) for j, k in zip(sel, kp) if k)
            tmax = max(abs(float(v[2])) for v, k in zip(ta, kp) if k)
            u = out[f"{key}/rays_c"][:3] - np.array(out[f"{key}/ref"][:3])[:, None]
            un = np.linalg.norm(u, axis=0)[kp]
            if planar:
                d = out[f"{key}/rays_c"][3:6][:, kp]
                en = np.abs((d * np.array(out[f"{key}/ref"][5:8])[:, None]).sum(axis=0))
                H, G = float((1.0 / en).max()), float((un / en ** 2).max())
            else:
                R = float(ref["R"])
                h = 1.0 + un / np.sqrt(R * R - un * un)
                H, G = float(h.max()), float((un * h).max())
            S = max(path, w["n_image"] * float(ref["R"]), abs(float(ref["opd_ref"]))) / wl
            out[f"{key}/scales"] = np.array(
                [S, max(tmax, float(np.abs(pup_a[:, kp]).max())), H, G, tmax])
            # the twelve moments of (a) and (b), over every ray of the field
            inten = [rows[j][-1][6] for j in sel]
            for lab, tt in (("a", ta), ("b", tb)):
                out[f"{key}/moments_{lab}"] = np.array(_fl(F.opd_sums(
                    mp, inten, [v[0] for v in tt], [v[1][0] for v in tt], [v[1][1] for v in tt])))
    assert mp.dps == DPS
    return out


def _job(args):
    kind, name = args
    return make_gen(name) if kind == "gen" else make_trace(name)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=F.GOLD)
    args = ap.parse_args()
    jobs = [("trace", c) for c in F.TRACE_CASES] + [("gen", c) for c in F.GEN_CASES]
    made = {}
    with multiprocessing.Pool(args.jobs) as pool:
        for (kind, name), part in zip(jobs, pool.imap(_job, jobs)):
            made.update(part)
            if kind == "trace":
                keep = part[f"trace/{name}/keep"]
                print(f"{name:42s} kept {int(keep.sum())}/{keep.size}  image yard f64/f32 "
                      f"{part[f'trace/{name}/f64/yard'][-1, 0]:.2e} / "
                      f"{part[f'trace/{name}/f32/yard'][-1, 0]:.2e}", flush=True)
            else:
                print(f"{name:42s} generated", flush=True)
    np.savez_compressed(args.out, **made)
    print(f"{args.out}: {os.path.getsize(args.out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
