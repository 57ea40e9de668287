"""`ol_zernike_fit`, `ol_zernike_eval`, `ol_sampled_mtf` on the device: the fixture of
tools/make_golden_zernike.py (the reference on CPU; this file never imports the reference), the
smallest shapes at which the kernels can go wrong, the stand-alone classes and the two seams.

Every bound comes from the reference: three times its own NumPy-to-torch spread, stored per case,
never below the first-order perturbation bound cond_2(A) K 2^-52 max|c| of the least-squares
problem (fit) or the rounding bound n 2^-52 of the normalised n-term sum (sampled MTF).  Each
test prints its measured figure before it asserts."""

import sys
import types

import numpy as np
import pytest
import torch

from optiland_amd import _capi, load_system
from optiland_amd import tracer as tr
from optiland_amd import zernike as Z
from optiland_amd.engine import sampled_mtf, zernike_eval, zernike_fit
from optiland_amd.mtf import SampledMTF
from optiland_amd.wavefront import ZernikeOPD
from tests import _zernike_fit as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = M.golden()
TILE, MAX_BLOCKS = 32, 256      # kZkTile, kZkMaxBlocks (csrc/zernike_fit.hip)
CHUNK, MAX_CHUNKS = 256, 256    # kZkBlock, kSmtfMaxChunks


def _dev(v, dtype=torch.float64):
    return torch.as_tensor(np.asarray(v), device=DEV, dtype=dtype)


def _fit(x, y, z, kind, k, intensity=None):
    c, status = zernike_fit(_dev(x), _dev(y), _dev(z), kind, k,
                            intensity=None if intensity is None else _dev(intensity), device=DEV)
    return c.cpu().numpy(), int(status)


def _disc(n, seed):
    rng = np.random.default_rng(seed)
    r, th = np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    return r * np.cos(th), r * np.sin(th)


def _surface(x, y):
    """A smooth wavefront that no finite Zernike sum reproduces."""
    return 0.8 * np.cos(3.0 * x + 1.0) * np.exp(-y * y) + 0.5 * x * y + 0.3 * (x * x + y * y) ** 2


# ------------------------------------------------------------------ 1. the fit, golden cases
@pytest.mark.parametrize("case", M.names(GOLD, "fit_cases"))
def test_fit_matches_the_reference_coefficients(case):
    x, y, z, kind, k = M.fit_inputs(GOLD, case)
    got, status = _fit(x, y, z, kind, k)
    want = GOLD[f"{case}/coeffs"]
    assert status == 0 and got.shape == want.shape
    err = float(np.abs(got - want).max())
    bound = M.fit_bound(GOLD[f"{case}/spread"], GOLD[f"{case}/cond"], k, np.abs(want).max())
    print(f"\n[fit] {case}: max |device - reference| = {err:.3e} (bound {bound:.3e}, "
          f"spread {float(GOLD[case + '/spread']):.3e})")
    assert err <= bound, (case, err, bound)


def _against_lstsq(tag, x, y, z, kind, k, intensity=None):
    got, status = _fit(x, y, z, kind, k, intensity)
    want, cond = M.numpy_fit(x, y, z, kind, k, intensity)
    assert status == 0, (tag, status)
    err = float(np.abs(got - want).max())
    # (no stored spread for a made-up problem: the floor of the bound alone)
    bound = M.fit_bound(0.0, cond, k, np.abs(want).max())
    print(f"\n[fit] {tag}: max |device - lstsq| = {err:.3e} (bound {bound:.3e}, cond {cond:.1f})")
    assert err <= bound, (tag, err, bound)
    return got


def test_one_point_one_term():
    got, status = _fit([0.3], [-0.2], [1.75], "fringe", 1)
    assert status == 0 and got.tolist() == [1.75]


@pytest.mark.parametrize("kind", Z.KINDS)
def test_as_many_points_as_terms(kind):
    # a hexapolar ring pattern of exactly 10 points: the centre, 3 and 6 on two rings
    th3, th6 = 2 * np.pi * np.arange(3) / 3 + 0.2, 2 * np.pi * np.arange(6) / 6
    x = np.concatenate([[0.0], 0.5 * np.cos(th3), 0.95 * np.cos(th6)])
    y = np.concatenate([[0.0], 0.5 * np.sin(th3), 0.95 * np.sin(th6)])
    _against_lstsq(f"n = K = 10 {kind}", x, y, _surface(x, y), kind, 10)


def test_one_point_fewer_than_terms_sets_the_status():
    x, y = _disc(9, 1)
    got, status = _fit(x, y, _surface(x, y), "fringe", 10)
    assert status & _capi.ZK_TOO_FEW
    assert np.isnan(got).all()       # not to be used, and not garbage
    # dark points do not count
    x, y = _disc(12, 2)
    inten = np.ones(12)
    inten[:3] = 0.0
    got, status = _fit(x, y, _surface(x, y), "fringe", 10, inten)
    assert status & _capi.ZK_TOO_FEW and np.isnan(got).all()


def test_seven_points_four_terms():
    x, y, z, kind, k = M.fit_inputs(GOLD, "hex1_fringe_4")
    assert x.size == 7 and k == 4 and x[0] == 0.0 and y[0] == 0.0   # (0, 0) is a sample
    _against_lstsq("7 x 4", x, y, z, kind, k)


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1,
                               TILE * MAX_BLOCKS - 1, TILE * MAX_BLOCKS, TILE * MAX_BLOCKS + 1,
                               2 * TILE * MAX_BLOCKS + 1])
def test_point_counts_around_the_tile_and_the_block_count(n):
    x, y = _disc(n, n)
    x[0] = y[0] = 0.0
    _against_lstsq(f"n = {n}", x, y, _surface(x, y), "fringe", 16)


def test_an_intensity_plane_with_zeros_fits_the_lit_points():
    """Not bit for bit the fit of the compacted arrays: a dark point is a row of zeros in ITS
    tile, so the lit points are grouped into tiles and blocks differently than after compaction,
    and the partial sums are added in another order.  Both are held to the bound."""
    x, y = _disc(1500, 5)
    z = _surface(x, y)
    inten = np.ones_like(x)
    inten[::3] = 0.0
    inten[7] = -1.0
    z[::3] = 1e6         # what a dark point holds must not matter
    masked = _against_lstsq("masked", x, y, z, "noll", 37, inten)
    keep = inten > 0
    packed, status = _fit(x[keep], y[keep], z[keep], "noll", 37)
    want, cond = M.numpy_fit(x, y, z, "noll", 37, inten)
    assert status == 0
    bound = M.fit_bound(0.0, cond, 37, np.abs(want).max())
    diff = float(np.abs(masked - packed).max())
    print(f"\n[fit] masked against compacted: {diff:.3e} (bound {bound:.3e})")
    assert diff <= 2 * bound


def test_a_nan_sets_the_status():
    x, y = _disc(300, 6)
    z = _surface(x, y)
    z[17] = np.nan
    got, status = _fit(x, y, z, "standard", 15)
    assert status & _capi.ZK_NONFINITE and np.isnan(got).all()
    # ... unless the point is dark
    inten = np.ones_like(x)
    inten[17] = 0.0
    got, status = _fit(x, y, z, "standard", 15, inten)
    assert status == 0 and np.isfinite(got).all()
    x[3] = np.inf
    assert _fit(x, y, z, "standard", 15, inten)[1] & _capi.ZK_NONFINITE


def test_rank_deficient_sets_the_status():
    """120 terms on the 127 points of six hexapolar rings: ten m = 0 radial polynomials on seven
    radii.  The reference answers with minimum-norm coefficients of 1e5 ... 1e7; normal
    equations cannot, and say so."""
    x, y, z = (GOLD[f"samp/hex6/{k}"] for k in "xyz")
    for kind in Z.KINDS:
        got, status = _fit(x, y, z, kind, 120)
        assert status == _capi.ZK_RANK_DEFICIENT, (kind, status)
        assert np.isnan(got).all()
    # every point at the origin: every m != 0 column is zero
    got, status = _fit(np.zeros(40), np.zeros(40), np.ones(40), "fringe", 4)
    assert status == _capi.ZK_RANK_DEFICIENT


def test_more_than_the_most_terms_is_refused():
    x, y = _disc(500, 7)
    with pytest.raises(ValueError, match="ZK_MAX_TERMS"):
        zernike_fit(_dev(x), _dev(y), _dev(x), "fringe", _capi.ZK_MAX_TERMS + 1, device=DEV)
    lib = _capi.load()
    t = _dev(x)
    rc = lib.ol_zernike_fit(_capi.ZK_MAX_TERMS + 1, t.data_ptr(), t.data_ptr(), 500, t.data_ptr(),
                            t.data_ptr(), t.data_ptr(), None, t.data_ptr(), t.data_ptr(), None)
    assert rc == -1 and b"OL_ZK_MAX_TERMS" in lib.ol_last_error()


# ------------------------------------------------------------------ 2. evaluation
@pytest.mark.parametrize("kind", Z.KINDS)
def test_eval_inside_on_and_outside_the_unit_circle(kind):
    rng = np.random.default_rng(11)
    k = _capi.ZK_MAX_TERMS
    c = rng.normal(0.0, 1.0, k)
    x, y = _disc(700, 12)
    # r = 1 exactly (also on the axes), r > 1, the origin
    x = np.concatenate([x, [1.0, 0.0, -1.0, 0.0, 0.6, 0.0, 1.2, -0.9]])
    y = np.concatenate([y, [0.0, 1.0, 0.0, -1.0, 0.8, 0.0, 0.5, -0.9]])
    got = zernike_eval(_dev(c), kind, _dev(x), _dev(y), device=DEV).cpu().numpy()
    A = Z.basis_numpy(kind, k, x, y)
    want = A @ c
    # two Horner evaluations of every radial polynomial (the kernel's with fused multiply-adds,
    # the host's without), each off by at most gamma_(2 s + 2) of the polynomial with its
    # coefficients made positive, then a K-term sum: (2 (2 s + 2) + K) 2^-52 sum |c_j| |Z|_j
    scale = M.abs_basis(kind, k, x, y) @ np.abs(c)
    limit = (2 * (2 * _capi.ZK_MAX_RADIAL + 2) + k) * M.EPS
    err = np.abs(got - want) / scale
    print(f"\n[eval] {kind}: max |device - host| / sum |c| |Z| = {err.max():.3e} "
          f"(bound {limit:.3e})")
    assert got.shape == x.shape and float(err.max()) <= limit
    # at the origin only the m = 0 terms are left
    m0 = [j for j, (_n, m) in enumerate(Z.indices(kind, k)) if m == 0]
    assert abs(got[-3] - float(A[-3, m0] @ c[m0])) <= limit * scale[-3]
    assert np.all(A[-3, [j for j in range(k) if j not in m0]] == 0.0)
    # shapes are kept
    grid = zernike_eval(_dev(c[:37]), kind, _dev(x[:12].reshape(3, 4)), _dev(y[:12].reshape(3, 4)),
                        device=DEV)
    assert grid.shape == (3, 4)


# ------------------------------------------------------------------ 3. the sampled MTF
def _smtf(g, case, shifts=None, **kw):
    return sampled_mtf(_dev(g[f"{case}/coeffs"]), str(g[f"{case}/kind"]), _dev(g[f"{case}/x"]),
                       _dev(g[f"{case}/y"]), _dev(g[f"{case}/opd"]), _dev(g[f"{case}/intensity"]),
                       _dev(g[f"{case}/shifts"] if shifts is None else shifts), device=DEV, **kw)


@pytest.mark.parametrize("case", M.names(GOLD, "smtf_cases"))
def test_sampled_mtf_from_given_inputs(case):
    want = GOLD[f"{case}/mtf"]
    mtf, otf = _smtf(GOLD, case, want_otf=True)
    got = mtf.cpu().numpy()
    assert got.shape == want.shape and otf.dtype == torch.complex128
    err = float(np.abs(got - want).max())
    bound = M.smtf_bound(GOLD[f"{case}/spread"], GOLD[f"{case}/x"].size)
    print(f"\n[smtf] {case}: {want.size} frequencies, max |device - reference| = {err:.3e} "
          f"(bound {bound:.3e}, spread {float(GOLD[case + '/spread']):.3e})")
    assert err <= bound, (case, err, bound)
    assert np.array_equal(otf.abs().cpu().numpy() > 0, got > 0)
    assert float(np.abs(otf.abs().cpu().numpy() - got).max()) <= 4 * M.EPS
    # the pupil function handed over instead of the OPD: the same sum
    p1 = np.sqrt(GOLD[f"{case}/intensity"]) * np.exp(2j * np.pi * GOLD[f"{case}/opd"])
    via = sampled_mtf(_dev(GOLD[f"{case}/coeffs"]), str(GOLD[f"{case}/kind"]),
                      _dev(GOLD[f"{case}/x"]), _dev(GOLD[f"{case}/y"]), None,
                      _dev(GOLD[f"{case}/intensity"]), _dev(GOLD[f"{case}/shifts"]),
                      p1=_dev(p1, torch.complex128), device=DEV).cpu().numpy()
    assert float(np.abs(via - want).max()) <= bound


def test_zero_shift_a_far_shift_and_a_dark_pupil():
    case = "cooke_fringe"
    x, y, c = GOLD[f"{case}/x"], GOLD[f"{case}/y"], GOLD[f"{case}/coeffs"]
    kind, n = str(GOLD[f"{case}/kind"]), x.size
    # an OPD map that IS its fit: the unshifted overlap is the whole pupil
    opd = zernike_eval(_dev(c), kind, _dev(x), _dev(y), device=DEV)
    rng = np.random.default_rng(3)
    inten = _dev(rng.uniform(0.2, 1.0, n))
    shifts = _dev([[0.0, 0.0], [3.0, 0.0], [0.0, -3.0], [2.2, 2.2]])
    got = sampled_mtf(_dev(c), kind, _dev(x), _dev(y), opd, inten, shifts, device=DEV).tolist()
    print(f"\n[smtf] zero shift: 1 - mtf = {1.0 - got[0]:.3e} (bound {n * M.EPS:.3e})")
    assert abs(got[0] - 1.0) <= n * M.EPS
    assert got[1:] == [0.0, 0.0, 0.0]          # every shifted point is outside: exactly 0
    dark = sampled_mtf(_dev(c), kind, _dev(x), _dev(y), opd, torch.zeros_like(inten),
                       shifts[:2], device=DEV).tolist()
    assert dark == [0.0, 0.0]                  # sampled.py:199-200
    one = sampled_mtf(_dev(c), kind, _dev(x), _dev(y), opd, inten, shifts[:1], device=DEV)
    assert one.shape == (1,) and one.tolist() == got[:1]
    none = sampled_mtf(_dev(c), kind, _dev(x), _dev(y), opd, inten, shifts[:0], device=DEV)
    assert none.shape == (0,)


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK * MAX_CHUNKS - 1,
                               CHUNK * MAX_CHUNKS, CHUNK * MAX_CHUNKS + 1])
def test_sampled_mtf_point_counts_around_the_chunk_and_the_chunk_count(n):
    rng = np.random.default_rng(n)
    x, y = _disc(n, n + 1)
    c = rng.normal(0.0, 0.3, 37)
    opd = M.numpy_eval(c, "fringe", x, y) + 0.01 * _surface(x, y)
    inten = rng.uniform(0.0, 1.0, n)
    shifts = np.array([[0.0, 0.0], [0.21, -0.13]]) if n > 4 * CHUNK else \
        np.array([[0.0, 0.0], [0.21, -0.13], [0.0, 0.7], [-1.1, 0.2], [0.05, 0.05]])
    got = sampled_mtf(_dev(c), "fringe", _dev(x), _dev(y), _dev(opd), _dev(inten), _dev(shifts),
                      device=DEV).cpu().numpy()
    want = M.numpy_sampled_mtf(c, "fringe", x, y, opd, inten, shifts)
    err = float(np.abs(got - want).max())
    print(f"\n[smtf] n = {n}: max |device - host| = {err:.3e} (bound {n * M.EPS:.3e})")
    assert err <= M.smtf_bound(0.0, n)


def test_bit_identical_from_run_to_run():
    x, y, z, kind, k = M.fit_inputs(GOLD, "uni32_fringe_120")
    big_x, big_y = _disc(2 * TILE * MAX_BLOCKS + 77, 21)
    for px, py, pz, kk in ((x, y, z, k), (big_x, big_y, _surface(big_x, big_y), 37)):
        runs = [_fit(px, py, pz, kind, kk)[0] for _ in range(3)]
        assert all(np.array_equal(runs[0], r) for r in runs[1:])
    c = _dev(GOLD["uni32_fringe_120/coeffs"])
    ev = [zernike_eval(c, kind, _dev(big_x), _dev(big_y), device=DEV) for _ in range(3)]
    assert all(torch.equal(ev[0], e) for e in ev[1:])
    ms = [_smtf(GOLD, "cooke_fringe") for _ in range(3)]
    assert all(torch.equal(ms[0], m) for m in ms[1:])
    # ... and a frequency's value does not depend on the frequencies it shares a call with
    alone = _smtf(GOLD, "cooke_fringe", GOLD["cooke_fringe/shifts"][5:6])
    assert alone[0] == ms[0][5]


# ------------------------------------------------------------------ 4. stand-alone classes
def _tracer(lens):
    return tr.HipRayTracer(load_system(M.SYSTEMS[lens]), DEV, dtype=torch.float64)


@pytest.mark.parametrize("kind,k", [("fringe", 37), ("noll", 37), ("standard", 120)])
def test_zernike_opd_fits_its_own_opd_map(kind, k):
    """Device coefficients against NumPy `lstsq` on the device's OWN OPD map, read back: the fit
    alone, without the trace's parity in the figure.  The spread is the fixture's for the same
    lens, field, sampling, kind and number of terms."""
    tracer = _tracer("cooke")
    w = float(GOLD["cooke_n32/wavelength"])
    z = ZernikeOPD(tracer, (0.0, 0.7), w, num_rings=15, zernike_type=kind, num_terms=k)
    assert z.coeffs.shape == (k,) and z.coeffs.dtype == torch.float64 and z.status == 0
    assert z.indices == Z.indices(kind, k) and z.num_pts == 721
    x, y, opd = (t.cpu().numpy() for t in (z.x, z.y, z.data.opd))
    want, cond = M.numpy_fit(x, y, opd, kind, k, z.data.intensity.cpu().numpy())
    err = float(np.abs(z.coeffs.cpu().numpy() - want).max())
    bound = M.fit_bound(GOLD[f"hex15_{kind}_{k}/spread"], cond, k, np.abs(want).max())
    print(f"\n[ZernikeOPD] {kind} {k}: max |device - lstsq(own map)| = {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound
    # the fixture's coefficients are those of the reference's OPD map: trace parity (2e-10
    # waves, README.md) enters, amplified by at most cond_2(A)
    far = float(np.abs(z.coeffs.cpu().numpy() - GOLD[f"hex15_{kind}_{k}/coeffs"]).max())
    assert far <= 1e-8
    fitted = z.poly(z.x, z.y)
    assert fitted.shape == z.x.shape
    host = M.numpy_eval(z.coeffs.cpu().numpy(), kind, x, y)
    assert float(np.abs(fitted.cpu().numpy() - host).max()) <= 1e-12


@pytest.mark.parametrize("case", M.names(GOLD, "e2e_cases"))
def test_standalone_sampled_mtf(case):
    tracer = _tracer(str(GOLD[f"{case}/system"]))
    m = SampledMTF(tracer, tuple(GOLD[f"{case}/field"]), float(GOLD[f"{case}/wavelength"]),
                   num_rays=int(GOLD[f"{case}/num_rays"]))
    assert m.xpd == pytest.approx(float(GOLD[f"{case}/xpd"]), rel=1e-12)
    assert m.xpl == pytest.approx(float(GOLD[f"{case}/xpl"]), rel=1e-12)
    got = m.calculate_mtf([tuple(f) for f in GOLD[f"{case}/freqs"]])
    want = GOLD[f"{case}/mtf"]
    assert isinstance(got, list) and len(got) == want.size
    err = float(np.abs(np.array([float(v) for v in got]) - want).max())
    bound = 3 * float(GOLD[f"{case}/spread"])
    print(f"\n[SampledMTF] {case}: max |stand-alone - reference| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (case, err, bound)


# ------------------------------------------------------------------ 5. the drop-in seams
class _Backend(types.ModuleType):
    _backends = {}

    @staticmethod
    def get_backend():
        return "torch"


class _Base:
    def __init__(self, coeffs):
        self.coeffs = coeffs


def _stand_in_modules():
    """`optiland.backend` and `optiland.zernike` as far as the seams ask them anything."""
    oz = types.ModuleType("optiland.zernike")
    for name in ("ZernikeFringe", "ZernikeStandard", "ZernikeNoll"):
        setattr(oz, name, type(name, (_Base,), {}))
    return {"optiland": types.ModuleType("optiland"), "optiland.backend": _Backend("be"),
            "optiland.zernike": oz}


@pytest.fixture
def stand_ins():
    from optiland_amd import analysis_seams as seams

    fake = _stand_in_modules()
    saved = {k: sys.modules.get(k) for k in fake}
    sys.modules.update(fake)
    calls = []
    had = {k: seams._ORIG.get(k) for k in ("zfit", "smtf")}
    seams._ORIG["zfit"] = lambda self: calls.append("zfit")
    seams._ORIG["smtf"] = lambda self, frequencies: calls.append("smtf") or "reference"
    try:
        yield seams, fake["optiland.zernike"], calls
    finally:
        for k, v in had.items():
            if v is None:
                seams._ORIG.pop(k, None)
            else:
                seams._ORIG[k] = v
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _fit_object(oz, case, cls="ZernikeFringe", dtype=torch.float64, **kw):
    x, y, z, _kind, k = M.fit_inputs(GOLD, case)
    me = types.SimpleNamespace(x=_dev(x, dtype), y=_dev(y, dtype), z=_dev(z, dtype),
                               zernike=getattr(oz, cls)(torch.ones(k, device=DEV, dtype=dtype)))
    me.__dict__.update(kw)
    return me


def test_fit_seam_serves_and_declines(stand_ins):
    seams, oz, calls = stand_ins
    for cls, kind in (("ZernikeFringe", "fringe"), ("ZernikeStandard", "standard"),
                      ("ZernikeNoll", "noll")):
        case = f"hex15_{kind}_37"
        me = _fit_object(oz, case, cls)
        before = dict(seams.STATS)
        assert seams._zernike_fit_fit(me) is None and not calls
        assert seams.STATS["zfit"] == before["zfit"] + 1
        assert seams.STATS["zfit_fallback"] == before["zfit_fallback"]
        c = me.zernike.coeffs
        assert c.device.type == "cuda" and c.dtype == torch.float64 and c.shape == (37,)
        want = GOLD[f"{case}/coeffs"]
        bound = M.fit_bound(GOLD[f"{case}/spread"], GOLD[f"{case}/cond"], 37, np.abs(want).max())
        assert float(np.abs(c.cpu().numpy() - want).max()) <= bound

    def declined(me, why):
        before = dict(seams.STATS)
        del calls[:]
        seams._zernike_fit_fit(me)
        assert calls == ["zfit"], why
        assert seams.STATS["zfit_fallback"] == before["zfit_fallback"] + 1, why
        assert seams.STATS["zfit"] == before["zfit"], why

    declined(_fit_object(oz, "hex6_fringe_37", dtype=torch.float32), "float32 tensors")
    me = _fit_object(oz, "hex6_fringe_37")
    me.zernike = type("Mine", (oz.ZernikeFringe,), {})(me.zernike.coeffs)
    declined(me, "a subclass")
    me = _fit_object(oz, "hex6_fringe_37")
    me.zernike.coeffs = torch.ones(_capi.ZK_MAX_TERMS + 1, device=DEV, dtype=torch.float64)
    declined(me, "too many terms")
    me = _fit_object(oz, "hex6_fringe_37")
    me.z = me.z.clone().requires_grad_(True)
    declined(me, "autograd")
    me = _fit_object(oz, "hex6_fringe_37")
    me.x = me.x.cpu()
    declined(me, "off the device")
    me = _fit_object(oz, "hex6_fringe_37")        # rank deficient: 120 terms on 127 points
    me.zernike.coeffs = torch.ones(120, device=DEV, dtype=torch.float64)
    declined(me, "rank deficient")
    me = _fit_object(oz, "hex6_fringe_37")
    me.z = me.z.clone()
    me.z[5] = float("nan")
    declined(me, "non-finite")


def _mtf_object(oz, case, cls=None, **kw):
    g = GOLD
    kind = str(g[f"{case}/kind"])
    cls = cls or {"fringe": "ZernikeFringe", "standard": "ZernikeStandard",
                  "noll": "ZernikeNoll"}[kind]
    inten, opd = _dev(g[f"{case}/intensity"]), _dev(g[f"{case}/opd"])
    me = types.SimpleNamespace(
        zernike_fit=types.SimpleNamespace(zernike=getattr(oz, cls)(_dev(g[f"{case}/coeffs"]))),
        x_norm=_dev(g[f"{case}/x"]), y_norm=_dev(g[f"{case}/y"]), intensity=inten,
        P1=torch.sqrt(inten) * torch.exp(2j * np.pi * opd),
        # shifts = xpl * (wavelength * 1e-3 * f) / (xpd / 2): frequencies that ARE the shifts
        wavelength=1000.0, xpd=2.0, xpl=1.0)
    me.__dict__.update(kw)
    return me


def test_sampled_mtf_seam_serves_and_declines(stand_ins):
    seams, oz, calls = stand_ins
    for case in M.names(GOLD, "smtf_cases"):
        me = _mtf_object(oz, case)
        before = dict(seams.STATS)
        got = seams._sampled_mtf_calculate(me, [tuple(s) for s in GOLD[f"{case}/shifts"]])
        assert not calls and seams.STATS["smtf"] == before["smtf"] + 1
        assert seams.STATS["smtf_fallback"] == before["smtf_fallback"]
        want = GOLD[f"{case}/mtf"]
        assert isinstance(got, list) and len(got) == want.size
        assert all(v.ndim == 0 and v.device.type == "cuda" and v.dtype == torch.float64
                   for v in got)
        bound = M.smtf_bound(GOLD[f"{case}/spread"], GOLD[f"{case}/x"].size)
        assert float(np.abs(np.array([float(v) for v in got]) - want).max()) <= bound
    # what the user replaced is what is used: other coefficients, another pupil function
    case = "cooke_fringe"
    me = _mtf_object(oz, case)
    me.zernike_fit.zernike.coeffs = me.zernike_fit.zernike.coeffs * 0.5
    me.P1 = me.P1 * torch.exp(2j * np.pi * 0.1 * me.x_norm)
    freqs = [tuple(s) for s in GOLD[f"{case}/shifts"][:6]]
    got = np.array([float(v) for v in seams._sampled_mtf_calculate(me, freqs)])
    want = M.numpy_sampled_mtf(0.5 * GOLD[f"{case}/coeffs"], "fringe", GOLD[f"{case}/x"],
                               GOLD[f"{case}/y"], GOLD[f"{case}/opd"] + 0.1 * GOLD[f"{case}/x"],
                               GOLD[f"{case}/intensity"], GOLD[f"{case}/shifts"][:6])
    assert float(np.abs(got - want).max()) <= M.smtf_bound(0.0, GOLD[f"{case}/x"].size)
    # a tensor of frequency pairs is read as the reference's loop reads it
    as_tensor = seams._sampled_mtf_calculate(_mtf_object(oz, case), _dev(GOLD[f"{case}/shifts"][:6]))
    assert len(as_tensor) == 6 and not calls

    def declined(me, freqs, why):
        before = dict(seams.STATS)
        del calls[:]
        assert seams._sampled_mtf_calculate(me, freqs) == "reference", why
        assert calls == ["smtf"], why
        assert seams.STATS["smtf_fallback"] == before["smtf_fallback"] + 1, why
        assert seams.STATS["smtf"] == before["smtf"], why

    declined(_mtf_object(oz, case, xpd=0.0), freqs, "xpd == 0")
    me = _mtf_object(oz, case)
    me.intensity = me.intensity.clone().requires_grad_(True)
    declined(me, freqs, "autograd")
    me = _mtf_object(oz, case)
    me.x_norm = me.x_norm.cpu()
    declined(me, freqs, "off the device")
    me = _mtf_object(oz, case)
    me.zernike_fit.zernike = type("Mine", (oz.ZernikeFringe,), {"poly": lambda s, r, p: 0})(
        me.zernike_fit.zernike.coeffs)
    declined(me, freqs, "a subclass overriding poly")
    declined(_mtf_object(oz, case), [(_dev([1.0, 2.0]), 0.0)], "non-scalar frequencies")


def test_uninstall_restores_the_originals(stand_ins):
    """enable() / disable() on stand-in reference modules: both seams go in with the signature
    they were written against and come out again."""
    seams, _oz, _calls = stand_ins
    fit_mod, mtf_mod = types.ModuleType("optiland.zernike.fit"), types.ModuleType("optiland.mtf.sampled")

    class ZernikeFit:
        def _fit(self):
            return "stock"

    class SampledMTF:
        def calculate_mtf(self, frequencies):
            return "stock"

    fit_mod.ZernikeFit, mtf_mod.SampledMTF = ZernikeFit, SampledMTF
    stock = (ZernikeFit.__dict__["_fit"], SampledMTF.__dict__["calculate_mtf"])
    keep_orig, keep_seams, keep_skipped = dict(seams._ORIG), dict(seams._SEAMS), dict(seams.SKIPPED)
    fake = {"optiland.zernike.fit": fit_mod, "optiland.mtf": types.ModuleType("optiland.mtf"),
            "optiland.mtf.sampled": mtf_mod}
    saved = {k: sys.modules.get(k) for k in fake}
    sys.modules.update(fake)
    try:
        seams._ORIG.clear()
        for k in list(seams._SEAMS):
            if k not in ("zfit", "smtf"):
                del seams._SEAMS[k]
        seams.enable()
        assert not seams.SKIPPED
        assert ZernikeFit.__dict__["_fit"] is seams._zernike_fit_fit
        assert SampledMTF.__dict__["calculate_mtf"] is seams._sampled_mtf_calculate
        assert seams._ORIG["zfit"] is stock[0] and seams._ORIG["smtf"] is stock[1]
        seams.disable()
        assert (ZernikeFit.__dict__["_fit"], SampledMTF.__dict__["calculate_mtf"]) == stock
        assert not seams._ORIG
    finally:
        seams._SEAMS.clear()
        seams._SEAMS.update(keep_seams)
        seams._ORIG.clear()
        seams._ORIG.update(keep_orig)
        seams.SKIPPED.clear()
        seams.SKIPPED.update(keep_skipped)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
