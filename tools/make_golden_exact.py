#!/usr/bin/env python
"""tests/golden/exact_zernike.npz, exact_huygens.npz, exact_smtf.npz: the analysis kernels'
operations evaluated with mpmath at 50 digits from fp64 inputs and rounded to fp64 once, for
tests/test_gpu_zernike_conditioning.py, test_gpu_zernike_exact.py and test_gpu_huygens_exact.py.

Nothing here shares code with what it checks:
  basis    Z_j = norm R_n^|m|(r) cos(m phi) / sin(|m| phi), phi = atan2(y, x), R from the factorial
           formula, (n, m) from `zernike.indices`, norm 1 (fringe) or sqrt((2n + 2) / (1 + [m = 0]));
  fit      the exact least-squares solution for that basis at the fp64 (x, y) and the fp64 z
           (normal equations: the Gram matrix summed exactly in 170-bit fixed point, solved at
           50 digits -- cond^2 <= 1e26 leaves more than 20 of them);
  Huygens  sum_j a_j exp(i k (R - opd_j)) / R * 1/2 (1 + ((P - Q_j) . Q_j / Rp) / R), k = 2 pi /
           lambda, term by term;
  sampled  sum_i I_i [r_i <= 1] exp(2 pi i (opd_i - W(x_i - dx, y_i - dy))) / sum_i I_i, the
           overlap sum of the reference's SampledMTF.calculate_mtf; the shifted coordinates are
           the fp64 differences (one IEEE operation, the same everywhere), W is exact.
Each fixture also holds the error of the suite's fp64 NumPy stand-in against that truth: the
tests' bounds are set against it, and the Huygens and sampled-MTF cases are only worth having
where the stand-in is worse than the bound the kernel is held to.

Fixed seeds; the .npz members are written uncompressed with a constant time stamp, so a rerun
reproduces the files byte for byte.

    python tools/make_golden_exact.py [zernike] [huygens] [smtf]      (CPU only, needs mpmath)
"""

from __future__ import annotations

import io
import math
import os
import sys
import zipfile
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.dont_write_bytecode = True
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402

from optiland_amd import zernike as Z  # noqa: E402
from tests import _exact as E  # noqa: E402
from tests import _huygens as H  # noqa: E402
from tests import _zernike_fit as M  # noqa: E402

mp.mp.dps = 50
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXED = 170                      # bits of the fixed-point Gram sums (2^-170 = 6.7e-52)
EPS = 2.0 ** -52

# (kind, K, rho) of the conditioning ladder and the rho of the threshold window (fringe 37)
LADDER = [("fringe", 37, 1.0), ("fringe", 37, 0.8), ("fringe", 37, 0.65), ("fringe", 37, 0.55),
          ("fringe", 37, 0.5), ("standard", 28, 0.65), ("standard", 28, 0.5), ("standard", 28, 0.4)]
WINDOW = [0.45, 0.44, 0.43, 0.42, 0.41, 0.40]
MASKED = ("fringe", 37, 0.65)
SMTF_WAVES = [0.3, 30.0, 300.0]
SMTF_RAISED = [1000.0, 3000.0]   # tried in turn while the stand-in stays inside the bound
SMTF_SHIFTS = [[0.0, 0.0], [0.21, -0.13], [0.0, 0.7], [-1.1, 0.2], [0.05, 0.05]]
HUYGENS_CASES = ["golden", "lambda_10p6um", "lambda_193nm", "rp_negative", "defocus_5mm",
                 "off_axis_20mm", "dark_samples"]
# pupil samples per case: the stand-in's error grows with sqrt(n), the bound with n (n + 32), so
# the long wavelength (k R 20 times smaller) takes fewer samples to stay a case worth having
HUYGENS_PUPIL, HUYGENS_IMAGE = {"lambda_10p6um": 48}, 8


# ------------------------------------------------------------------ writing
def save(path, arrays):
    """An .npz that `np.load` reads, byte for byte the same on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def f64(v):
    return np.array([float(e) for e in v], dtype=np.float64)


# ------------------------------------------------------------------ the basis
def _radial(n, a):
    f = math.factorial
    return [(-1) ** k * f(n - k) // (f(k) * f((n + a) // 2 - k) * f((n - a) // 2 - k))
            for k in range((n - a) // 2 + 1)]


def _norm(kind, n, m):
    return mp.mpf(1) if kind == "fringe" else mp.sqrt(mp.mpf(2 * n + 2) / (2 if m == 0 else 1))


def mp_basis(kind, num_terms, x, y, absolute=False):
    """[[Z_j(x_i, y_i)]] as mpf, (points, K).  `absolute`: norm sum_k |c_k| r^(n - 2k) instead
    (what `_zernike_fit.abs_basis` restates in fp64)."""
    idx = Z.indices(kind, num_terms)
    top = max(n for n, _m in idx)
    rad = {(n, abs(m)): _radial(n, abs(m)) for n, m in idx}
    norm = [_norm(kind, n, m) for n, m in idx]
    rows = []
    for xv, yv in zip(np.asarray(x, dtype=np.float64).reshape(-1),
                      np.asarray(y, dtype=np.float64).reshape(-1)):
        X, Y = mp.mpf(float(xv)), mp.mpf(float(yv))
        r = mp.sqrt(X * X + Y * Y)
        phi = mp.atan2(Y, X)
        rp = [mp.mpf(1)]
        for _ in range(top):
            rp.append(rp[-1] * r)
        ang = {}
        row = []
        for j, (n, m) in enumerate(idx):
            a = abs(m)
            if absolute:
                row.append(norm[j] * mp.fsum(abs(c) * rp[n - 2 * k]
                                             for k, c in enumerate(rad[(n, a)])))
                continue
            if m not in ang:
                ang[m] = mp.cos(m * phi) if m >= 0 else mp.sin(a * phi)
            R = mp.fsum(c * rp[n - 2 * k] for k, c in enumerate(rad[(n, a)]))
            row.append(norm[j] * R * ang[m])
        rows.append(row)
    return rows


# ------------------------------------------------------------------ the fit
def surface(x, y):
    """tests/test_gpu_zernike_fit.py:_surface -- a wavefront no finite Zernike sum reproduces."""
    return 0.8 * np.cos(3.0 * x + 1.0) * np.exp(-y * y) + 0.5 * x * y + 0.3 * (x * x + y * y) ** 2


def ladder_points(rho, n=300):
    rng = np.random.default_rng(0)
    r = np.sqrt(rng.random(n))
    th = 2 * np.pi * rng.random(n)
    x, y = rho * r * np.cos(th), rho * r * np.sin(th)
    return x, y, surface(x, y)


def mp_fit(rows, z):
    """The exact least-squares coefficients: rows (points, K) of mpf, z fp64."""
    K = len(rows[0])
    one = mp.mpf(2) ** FIXED
    A = [[int(mp.nint(v * one)) for v in row] for row in rows]
    zi = [int(mp.nint(mp.mpf(float(v)) * one)) for v in z]
    G = mp.matrix(K, K)
    b = mp.matrix(K, 1)
    scale = mp.mpf(2) ** (-2 * FIXED)
    cols = list(zip(*A))
    for p in range(K):
        for q in range(p, K):
            s = sum(u * v for u, v in zip(cols[p], cols[q]))
            G[p, q] = G[q, p] = mp.mpf(s) * scale
        b[p] = mp.mpf(sum(u * v for u, v in zip(cols[p], zi))) * scale
    return list(mp.cholesky_solve(G, b))


def min_scaled_pivot(A):
    """The smallest pivot of the Cholesky factorisation of D A^T A D, D = diag(A^T A)^-1/2, in
    fp64 NumPy: where the kernel's pivot test stands for a problem (the device's own sums
    differ in the last digits).  NaN once a pivot is not positive."""
    G = A.T @ A
    d = 1.0 / np.sqrt(np.diag(G))
    S = G * d[:, None] * d[None, :]
    K = S.shape[0]
    low = np.inf
    for j in range(K):
        if not S[j, j] > 0.0:
            return float("nan")
        low = min(low, S[j, j])
        S[j + 1:, j] /= math.sqrt(S[j, j])
        S[j + 1:, j + 1:] -= np.outer(S[j + 1:, j], S[j + 1:, j])
    return float(low)


def fit_case(kind, num_terms, rho, masked=False):
    x, y, z = ladder_points(rho)
    out = {"x": x, "y": y, "kind": np.array(kind), "num_terms": np.array(num_terms),
           "rho": np.array(rho)}
    keep = np.ones(x.size, dtype=bool)
    if masked:      # every third point dark, garbage where it is dark
        inten = np.ones_like(x)
        inten[::3] = 0.0
        z = z.copy()
        z[::3] = 1e6
        keep = inten > 0
        out["intensity"] = inten
    out["z"] = z
    rows = mp_basis(kind, num_terms, x[keep], y[keep])
    exact = f64(mp_fit(rows, z[keep]))
    A = np.array([[float(v) for v in row] for row in rows])
    lstsq, _cond = M.numpy_fit(x, y, z, kind, num_terms, out.get("intensity"))
    out["coeffs"] = exact
    out["cond"] = np.array(float(np.linalg.cond(A)))
    out["min_pivot"] = np.array(min_scaled_pivot(A))
    out["numpy_err"] = np.array(float(np.abs(lstsq - exact).max()))
    return out


def fit_name(kind, num_terms, rho, masked=False):
    return f"fit/{kind}{num_terms}_rho{rho:g}" + ("_masked" if masked else "")


# ------------------------------------------------------------------ evaluation
def eval_points():
    """61 points: the origin, r = 1 on the axes and at (0.6, 0.8), r = 1.2, r = 1e-8, the disc."""
    rng = np.random.default_rng(41)
    r, th = np.sqrt(rng.random(48)), 2 * np.pi * rng.random(48)
    x = [0.0, 1.0, 0.0, -1.0, 0.0, 0.6, 1.2, 0.0, -0.72, 1e-8, 0.0, -6e-9, 0.96]
    y = [0.0, 0.0, 1.0, 0.0, -1.0, 0.8, 0.0, -1.2, 0.96, 0.0, 1e-8, 8e-9, -0.72]
    return np.concatenate([x, r * np.cos(th)]), np.concatenate([y, r * np.sin(th)])


def eval_case(kind, num_terms=120):
    x, y = eval_points()
    rng = np.random.default_rng(43)
    c = rng.normal(0.0, 1.0, num_terms)
    idx = Z.indices(kind, num_terms)
    top_n = max(range(num_terms), key=lambda j: (idx[j][0], -j))
    top_m = max(range(num_terms), key=lambda j: (abs(idx[j][1]), -j))
    rows = mp_basis(kind, num_terms, x, y)
    A = np.array([[float(v) for v in row] for row in rows])
    want = f64(mp.fsum(mp.mpf(float(cj)) * v for cj, v in zip(c, row)) for row in rows)
    scale = np.array([[float(v) for v in row]
                      for row in mp_basis(kind, num_terms, x, y, absolute=True)])
    host = Z.basis_numpy(kind, num_terms, x, y)
    assert np.all(host[scale == 0.0] == 0.0) and np.all(A[scale == 0.0] == 0.0)
    rel = np.abs(host - A)[scale > 0.0] / scale[scale > 0.0]
    return {"x": x, "y": y, "c": c, "basis": A, "want": want, "abs_basis": scale,
            "top_n": np.array(top_n), "top_m": np.array(top_m),
            "numpy_err": np.array(float(rel.max()))}


def make_zernike(only=None):
    out = {"ladder": np.array([fit_name(*c) for c in LADDER]),
           "window": np.array([fit_name("fringe", 37, r) for r in WINDOW]),
           "masked": np.array(fit_name(*MASKED, masked=True)), "kinds": np.array(Z.KINDS)}
    jobs = [(fit_name(*c), lambda c=c: fit_case(*c)) for c in LADDER]
    jobs += [(fit_name("fringe", 37, r), lambda r=r: fit_case("fringe", 37, r)) for r in WINDOW]
    jobs += [(fit_name(*MASKED, masked=True), lambda: fit_case(*MASKED, masked=True))]
    jobs += [(f"eval/{k}", lambda k=k: eval_case(k)) for k in Z.KINDS]
    for name, job in jobs:
        if only is not None and name != only:
            continue
        for key, v in job().items():
            out[f"{name}/{key}"] = v
        if name.startswith("fit/"):
            print(f"{name}: cond {float(out[name + '/cond']):.3e}, min scaled pivot "
                  f"{float(out[name + '/min_pivot']):.2e}, lstsq off by "
                  f"{float(out[name + '/numpy_err']):.2e}")
        else:
            print(f"{name}: basis_numpy off by {float(out[name + '/numpy_err']):.2e} of "
                  f"norm sum |c_k| r^(n-2k)")
    return out


# ------------------------------------------------------------------ Huygens
def huygens_args(case):
    """(image_x, image_y, image_z, pupil_x, pupil_y, pupil_z, amp, opd, wavelength, Rp)"""
    ix, iy, iz, px, py, pz, amp, opd, wl, rp = H.random_case(
        HUYGENS_PUPIL.get(case, 150), HUYGENS_IMAGE, complex_amp=True, seed=97)
    if case == "lambda_10p6um":
        wl = 10.6e-3
    elif case == "lambda_193nm":
        wl = 0.193e-3
    elif case == "rp_negative":     # the cap and the image mirrored in the pupil's vertex plane
        pz, iz, rp = 2 * 6.08 - pz, 2 * 6.08 - iz, -rp
    elif case == "defocus_5mm":
        iz = iz + 5.0
    elif case == "off_axis_20mm":
        iy = iy + 20.0
    elif case == "dark_samples":
        amp = amp.copy()
        amp[::4] = 0.0
    elif case != "golden":
        raise ValueError(case)
    return ix, iy, iz, px, py, pz, amp, opd, wl, rp


def mp_huygens(ix, iy, iz, px, py, pz, amp, opd, wl, rp):
    """(field (n_image,) complex128, scale (n_image,)): the exact sum rounded once, and
    sum_j |a_j q_mj / R_mj| per pixel."""
    k = 2 * mp.pi / mp.mpf(float(wl))
    Rp = mp.mpf(float(rp))
    Q = [(mp.mpf(float(u)), mp.mpf(float(v)), mp.mpf(float(w))) for u, v, w in zip(px, py, pz)]
    a = [mp.mpc(float(np.real(v)), float(np.imag(v))) for v in amp]
    o = [mp.mpf(float(v)) for v in opd]
    field, scale = [], []
    for X, Y, Zc in zip(ix, iy, iz):
        P = (mp.mpf(float(X)), mp.mpf(float(Y)), mp.mpf(float(Zc)))
        re, im, s = [], [], []
        for (u, v, w), aj, oj in zip(Q, a, o):
            dx, dy, dz = P[0] - u, P[1] - v, P[2] - w
            R = mp.sqrt(dx * dx + dy * dy + dz * dz)
            q = (1 + ((dx * u + dy * v + dz * w) / Rp) / R) / 2
            t = aj * mp.expj(k * (R - oj)) / R * q
            re.append(t.real)
            im.append(t.imag)
            s.append(abs(aj) * abs(q) / R)
        field.append(complex(float(mp.fsum(re)), float(mp.fsum(im))))
        scale.append(float(mp.fsum(s)))
    return np.array(field), np.array(scale)


def huygens_case(case):
    args = huygens_args(case)
    field, scale = mp_huygens(*args)
    err = np.abs(H.direct_field(*args) - field)
    bound = E.huygens_bound(args[3].size, scale)
    # the case is only worth having where fp64 without the low-order phase terms misses the
    # bound the kernel is held to
    assert float((err / bound).max()) > 1.0, (case, err, bound)
    out = dict(zip(H.ARGS, args))
    out.update(field=field, scale=scale, numpy_err=err)
    return out


def make_huygens(only=None):
    out = {"cases": np.array(HUYGENS_CASES)}
    for case in HUYGENS_CASES:
        if only is not None and case != only:
            continue
        got = huygens_case(case)
        for key, v in got.items():
            out[f"{case}/{key}"] = np.asarray(v)
        ratio = got["numpy_err"] / E.huygens_bound(got["pupil_x"].size, got["scale"])
        print(f"huygens {case}: NumPy direct sum off by {ratio.min():.1f} ... {ratio.max():.1f} "
              f"x the kernel's bound")
    return out


# ------------------------------------------------------------------ sampled MTF
def mp_sampled_mtf(rows_by_shift, inside_by_shift, coeffs, opd, inten, total=None):
    c = [mp.mpf(float(v)) for v in coeffs]
    total = mp.fsum(mp.mpf(float(v)) for v in inten) if total is None else mp.mpf(total)
    out = []
    for rows, inside in zip(rows_by_shift, inside_by_shift):
        terms = []
        for i, row in enumerate(rows):
            if not inside[i]:
                continue
            w = mp.fsum(cj * v for cj, v in zip(c, row))
            terms.append(mp.mpf(float(inten[i])) * mp.expj(2 * mp.pi * (mp.mpf(float(opd[i])) - w)))
        s = mp.fsum(t.real for t in terms) + 1j * mp.fsum(t.imag for t in terms)
        out.append(float(abs(s) / total))
    return np.array(out)


def smtf_inputs(n=257, num_terms=37):
    rng = np.random.default_rng(57)
    r, th = np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    x, y = r * np.cos(th), r * np.sin(th)
    c0 = rng.normal(0.0, 0.3, num_terms)
    opd0 = M.numpy_eval(c0, "fringe", x, y) + 0.01 * surface(x, y)
    inten = rng.uniform(0.2, 1.0, n)
    return x, y, c0, opd0, inten, np.array(SMTF_SHIFTS)


def make_smtf(only=None):
    x, y, c0, opd0, inten, shifts = smtf_inputs()
    kind = "fringe"
    out = {"x": x, "y": y, "intensity": inten, "shifts": shifts, "kind": np.array(kind)}
    rows_by_shift, inside_by_shift = [], []
    if only != "rim":
        for dx, dy in shifts:
            xs, ys = x - dx, y - dy
            rr = np.sqrt(xs ** 2 + ys ** 2)
            assert np.abs(rr - 1.0).min() > 1e-9          # no point whose side is in doubt
            inside_by_shift.append(~(rr > 1.0))
            rows_by_shift.append(mp_basis(kind, c0.size, xs, ys))
    names, beaten = [], False
    for waves in SMTF_WAVES + SMTF_RAISED:
        name = f"waves{waves:g}"
        if waves in SMTF_RAISED and beaten:
            break
        if only not in (None, name):
            continue
        s = waves / np.abs(opd0).max()
        c, opd = s * c0, s * opd0
        want = mp_sampled_mtf(rows_by_shift, inside_by_shift, c, opd, inten)
        host = M.numpy_sampled_mtf(c, kind, x, y, opd, inten, shifts)
        err = float(np.abs(host - want).max())
        bound = E.smtf_bound(kind, c, x, y, opd, shifts)
        if waves >= SMTF_WAVES[-1]:
            beaten = err > bound
        names.append(name)
        out.update({f"{name}/coeffs": c, f"{name}/opd": opd, f"{name}/mtf": want,
                    f"{name}/numpy_err": np.array(err), f"{name}/bound": np.array(bound),
                    f"{name}/numpy_exceeds": np.array(err > bound)})
        print(f"smtf {name}: mtf {np.array2string(want, precision=4)}, NumPy stand-in off by "
              f"{err:.3e}, kernel bound {bound:.3e}")
    out["cases"] = np.array(names)
    if only is None or only == "rim":
        out.update(rim_case())
    return out


def _changes_side(xv, yv):
    """Does fl(fma(x, x, fl(y y))) or fl(fma(y, y, fl(x x))) decide `> 1` differently from
    fl(fl(x x) + fl(y y))?  Exact rationals, rounded once as an fma does."""
    fx, fy = Fraction(xv), Fraction(yv)
    plain = math.sqrt(xv * xv + yv * yv) > 1.0
    one = math.sqrt(float(fx * fx + Fraction(yv * yv))) > 1.0
    two = math.sqrt(float(fy * fy + Fraction(xv * xv))) > 1.0
    return one != plain or two != plain


def rim_case(num_terms=37):
    g = M.golden()
    hx, hy = g["samp/hex15/x"], g["samp/hex15/y"]
    on = np.abs(np.hypot(hx, hy) - 1.0) < 1e-12
    rng = np.random.default_rng(71)
    th = 2 * np.pi * rng.random(4096)
    cx, cy = np.cos(th), np.sin(th)
    # cos^2 + sin^2 of fp64 values never rounds to 1 + 2^-51, the first sum whose square root is
    # above 1, so those points alone are all inside whatever the contraction.  A second copy of
    # them, each coordinate moved outwards by one or two ulp, straddles that sum.
    bx, by = cx.copy(), cy.copy()
    for _ in range(2):
        move = rng.random(th.size) < 0.75
        bx = np.where(move, np.nextafter(bx, np.copysign(2.0, bx)), bx)
        move = rng.random(th.size) < 0.75
        by = np.where(move, np.nextafter(by, np.copysign(2.0, by)), by)
    x = np.concatenate([cx, hx[on], bx])
    y = np.concatenate([cy, hy[on], by])
    c = rng.normal(0.0, 0.3, num_terms)
    opd = M.numpy_eval(c, "fringe", x, y) + 0.05 * surface(x, y)
    inten = np.ones_like(x)
    inside = ~(np.sqrt(x ** 2 + y ** 2) > 1.0)         # NumPy's unfused decision
    flips = sum(_changes_side(float(a), float(b)) for a, b in zip(x, y))
    rows = mp_basis("fringe", num_terms, x[inside], y[inside])
    want = mp_sampled_mtf([rows], [np.ones(len(rows), dtype=bool)], c, opd[inside], inten[inside],
                          total=x.size)
    print(f"smtf rim: {x.size} points ({int(on.sum())} of hex15), {int(inside.sum())} inside by "
          f"the unfused test, {flips} change side under a fused one; mtf {want[0]:.6f}")
    return {"rim/x": x, "rim/y": y, "rim/coeffs": c, "rim/opd": opd, "rim/mtf": want,
            "rim/inside": np.array(int(inside.sum())), "rim/fused_flips": np.array(int(flips))}


MAKERS = {"zernike": make_zernike, "huygens": make_huygens, "smtf": make_smtf}


def main(argv):
    for name in argv or list(MAKERS):
        path = os.path.join(GOLDEN, f"exact_{name}.npz")
        save(path, MAKERS[name]())
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
