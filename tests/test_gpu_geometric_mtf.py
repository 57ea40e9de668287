"""`ol_geometric_mtf` (optiland_amd/csrc/mtf.hip) on the MI355X: the reference's own hits and
curves (tests/golden/geometric_mtf.npz, NumPy backend), random curves against `np.histogram` + a
NumPy fp64 sum, float32 planes, bit-reproducibility, the non-finite flag and the refusals, the
stand-alone `GeometricMTF` / `FFTMTF` and the drop-in seam -- all without the reference package.

Tolerances (every stored curve is compared at every frequency; each test prints its figure):

* counts: equal to `np.histogram`'s, exactly.
* MTF from GIVEN hits (golden and random curves): MEASURED_GIVEN below is the largest
  |kernel - NumPy| seen on the MI355X over all of them (profiles/geometric_mtf.txt: 9.96e-13, in
  the unscaled Cooke case; 1e-13 to 2e-13 in the scaled golden cases, 6e-16 for random curves
  about 0 and 5.7e-13 for random curves about 25 mm); the tests assert 10 x that, which must
  stay below the 1e-10 the arithmetic allows (a 257-term fp64 sum whose yardstick, NumPy's
  `cos(2 pi v x)` at |x| = 25 mm, itself rounds its argument to ~1e-11 rad).
* MTF from the project's OWN fp64 trace: the hits differ from the reference's by ~1e-12 mm on
  these conic-only lenses and a hit can cross a bin edge; jittering the reference's hits by a
  Gaussian of 1e-9 mm moves its own MTF by 4.7e-8 (Cooke) / 2.9e-8 (double Gauss)
  (`fp64_spread` in the fixture).  MEASURED_OWN_FP64 is the largest difference seen on the
  MI355X (1.10e-12, unscaled Cooke case; 3.5e-13 to 6.3e-13 otherwise: no hit changed its bin);
  the test asserts 10 x that, capped at 1e-6.
* fp32 tracer: the reference against itself, case by case, with its hits jittered by a
  Gaussian of 6e-6 mm, the documented fp32 hit parity, moves by 2.6e-4 (Cooke, max_freq 100) to
  3.3e-3 (double Gauss, 469 hexapolar hits); 3.6e-4 / 5.4e-4 in the two default cases
  (`fp32_spread` per case in the fixture, tools/make_golden_mtf.py).  The device is allowed
  3 x the spread of its case.  Measured on the MI355X: 0.5 (max_freq 100) to 1.4 (Cooke
  default: 4.9e-4) times the spread.
"""

import ctypes as C
import sys
import types

import numpy as np
import pytest
import torch

from optiland_amd import _capi, load_system
from optiland_amd import tracer as tr
from optiland_amd.engine import geometric_mtf, geometric_mtf_launch
from optiland_amd.mtf import FFTMTF, GeometricMTF
from tests import _geometric_mtf as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = M.golden()

MEASURED_GIVEN = 9.96e-13     # largest |kernel - NumPy| from given hits, measured on the MI355X
MEASURED_OWN_FP64 = 1.10e-12 # largest |stand-alone fp64 - golden|, measured on the MI355X
TOL_GIVEN = 10 * MEASURED_GIVEN
TOL_OWN_FP64 = min(10 * MEASURED_OWN_FP64, 1e-6)
assert TOL_GIVEN <= 1e-10


def _dev(v, dtype=None):
    return torch.as_tensor(np.asarray(v), device=DEV, dtype=dtype)


def _freq(n=256, top=360.0):
    return np.linspace(0.0, top, n)


# ------------------------------------------------------------------ 1. golden hits
@pytest.mark.parametrize("case", M.cases(GOLD))
def test_golden_hits_give_numpy_counts_and_the_reference_curves(case):
    curves = M.curves(GOLD, case)
    freq, scale = GOLD[f"{case}/freq"], M.scale_of(GOLD, case)
    mtf, counts, edges = geometric_mtf([_dev(c) for c in curves], _dev(freq),
                                       None if scale is None else _dev(scale), want_counts=True)
    counts, edges, mtf = counts.cpu().numpy(), edges.cpu().numpy(), mtf.cpu().numpy()
    want = GOLD[f"{case}/mtf"].reshape(mtf.shape)
    for c in range(len(curves)):
        tag = f"{'ts'[c % 2]}{c // 2}"
        assert np.array_equal(counts[c], GOLD[f"{case}/counts_{tag}"]), (case, tag)
        e = GOLD[f"{case}/edges_{tag}"]
        assert edges[c, 0] == e[0] and edges[c, 1] == e[-1]
    err = float(np.max(np.abs(mtf - want)))
    print(f"\n[given] {case}: max |kernel - reference| = {err:.3e}")
    assert err <= TOL_GIVEN, (case, err)


# ------------------------------------------------------------------ 2. random curves
def _random_curve(kind, n, offset, rng):
    if kind == "normal":
        x = 0.01 * rng.standard_normal(n)
    elif kind == "uniform":
        x = 0.05 * (rng.random(n) - 0.5)
    elif kind == "two-cluster":
        x = 0.002 * rng.standard_normal(n) + np.where(rng.random(n) < 0.3, -0.02, 0.02)
    elif kind == "equal":
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    return x + offset


def _plant_on_edges(x, n_bins, rng):
    """Overwrite a tenth of the points (at least the inner edges once, where they fit) with
    exact values of np.histogram's own edges; min and max stay."""
    if x.size < 4 or n_bins < 2 or x.min() == x.max():
        return x
    edges = np.histogram_bin_edges(x, bins=n_bins)
    keep = {int(np.argmin(x)), int(np.argmax(x))}
    free = np.array([i for i in range(x.size) if i not in keep]) if x.size < 5000 else \
        np.setdiff1d(np.arange(x.size), list(keep))
    k = min(free.size, max(x.size // 10, min(free.size, n_bins - 1)))
    where = rng.choice(free, size=k, replace=False)
    x = x.copy()
    x[where] = edges[1:-1][np.arange(k) % (n_bins - 1)]
    return x


@pytest.mark.parametrize("n", [1, 300, 7668, 1_000_000])
@pytest.mark.parametrize("offset", [0.0, 25.0])
def test_random_curves_match_numpy(n, offset):
    rng = np.random.default_rng(n + int(offset))
    freq = _freq()
    scale = 1.0 - 0.5 * freq / freq[-1]
    curves = []
    for kind in ("normal", "uniform", "two-cluster", "equal"):
        x = _random_curve(kind, n, offset, rng)
        curves += [x, _plant_on_edges(x, freq.size + 1, rng)]
    mtf, counts, edges = geometric_mtf([_dev(c) for c in curves], _dev(freq), _dev(scale),
                                       want_counts=True)
    mtf, counts, edges = mtf.cpu().numpy(), counts.cpu().numpy(), edges.cpu().numpy()
    worst = 0.0
    for c, x in enumerate(curves):
        want, A, e = M.direct_mtf(x, freq, scale)
        assert np.array_equal(counts[c], A), (n, offset, c)
        assert edges[c, 0] == e[0] and edges[c, 1] == e[-1]
        worst = max(worst, float(np.max(np.abs(mtf[c] - want))))
    print(f"\n[given] random n={n} offset={offset}: max |kernel - NumPy| = {worst:.3e}")
    assert worst <= TOL_GIVEN, (n, offset, worst)


@pytest.mark.parametrize("n_bins", [1, 2, 65, 1025, 4097, _capi.MTF_MAX_BINS])
def test_other_bin_counts(n_bins):
    rng = np.random.default_rng(n_bins)
    freq = _freq(33, 200.0)
    curves = [_plant_on_edges(_random_curve("normal", 20000, 3.0, rng), n_bins, rng),
              _random_curve("two-cluster", 777, -12.0, rng)]
    mtf, counts, _ = geometric_mtf([_dev(c) for c in curves], _dev(freq), None, n_bins,
                                   want_counts=True)
    for c, x in enumerate(curves):
        want, A, _e = M.direct_mtf(x, freq, None, n_bins)
        assert np.array_equal(counts[c].cpu().numpy(), A), (n_bins, c)
        assert float(np.max(np.abs(mtf[c].cpu().numpy() - want))) <= TOL_GIVEN


# ------------------------------------------------------------------ 3. float32 planes
def test_float32_planes_give_the_result_of_their_widened_values():
    rng = np.random.default_rng(32)
    freq = _freq()
    curves32 = [(_random_curve(kind, 7668, off, rng)).astype(np.float32)
                for kind, off in (("normal", 0.0), ("uniform", 25.0), ("two-cluster", -7.0))]
    got32 = geometric_mtf([_dev(c) for c in curves32], _dev(freq), want_counts=True)
    assert got32[0].dtype == torch.float64
    got64 = geometric_mtf([_dev(c.astype(np.float64)) for c in curves32], _dev(freq),
                          want_counts=True)
    for a, b in zip(got32, got64):
        assert torch.equal(a, b)
    for c, x in enumerate(curves32):
        want, A, _e = M.direct_mtf(x.astype(np.float64), freq)
        assert np.array_equal(got32[1][c].cpu().numpy(), A)
        assert float(np.max(np.abs(got32[0][c].cpu().numpy() - want))) <= TOL_GIVEN


# ------------------------------------------------------------------ 4. reproducibility
def test_bit_identical_from_run_to_run_and_alone_or_in_a_batch():
    rng = np.random.default_rng(4)
    freq = _dev(_freq())
    curves = [_dev(_random_curve(kind, n, off, rng)) for kind, n, off in
              (("normal", 7668, 0.0), ("uniform", 300, 25.0), ("two-cluster", 1_000_000, 3.0),
               ("equal", 50, 1.0), ("normal", 100_000, -9.0), ("uniform", 7668, 0.5))]
    a = geometric_mtf(curves, freq, want_counts=True)
    b = geometric_mtf(curves, freq, want_counts=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for c in (0, 2, 5):
        one = geometric_mtf([curves[c]], freq, want_counts=True)
        for u, v in zip(one, a):
            assert torch.equal(u[0], v[c]), c


# ------------------------------------------------------------------ 5. flags and refusals
def test_nan_flags_its_curve_only():
    rng = np.random.default_rng(5)
    freq = _freq()
    curves = [_random_curve("normal", 3000, 1.0, rng) for _ in range(4)]
    curves[1] = curves[1].copy()
    curves[1][1234] = np.nan
    curves[3] = curves[3].copy()
    curves[3][7] = np.inf
    mtf, counts, edges, flags = geometric_mtf_launch([_dev(c) for c in curves], _dev(freq))
    assert flags.tolist() == [0, _capi.MTF_NONFINITE, 0, _capi.MTF_NONFINITE]
    for c in (1, 3):
        assert torch.isnan(mtf[c]).all() and torch.isnan(edges[c]).all()
        assert int(counts[c].sum()) == 0
    for c in (0, 2):
        want, A, _e = M.direct_mtf(curves[c], freq)
        assert np.array_equal(counts[c].cpu().numpy(), A)
        assert float(np.max(np.abs(mtf[c].cpu().numpy() - want))) <= TOL_GIVEN
    with pytest.raises(ValueError, match="not finite"):
        geometric_mtf([_dev(c) for c in curves], _dev(freq))


def test_an_empty_curve_is_nan_without_a_flag():
    mtf, counts, edges, flags = geometric_mtf_launch(
        [_dev(np.zeros(0)), _dev(np.array([1.0, 2.0]))], _dev(_freq(8, 10.0)))
    assert flags.tolist() == [0, 0] and edges[0].tolist() == [0.0, 1.0]
    assert torch.isnan(mtf[0]).all() and int(counts[0].sum()) == 0
    assert float(mtf[1][0]) == 1.0


def test_refusals():
    lib = _capi.load()
    x = torch.zeros(16, dtype=torch.float64, device=DEV)
    f = torch.zeros(4, dtype=torch.float64, device=DEV)
    out = torch.zeros(64, dtype=torch.float64, device=DEV)
    iout = torch.zeros(64, dtype=torch.int32, device=DEV)
    ptrs = (C.c_void_p * 2)(x.data_ptr(), x.data_ptr())
    lens = (C.c_int64 * 2)(16, 16)

    def call(dt=_capi.F64, k=2, coords=ptrs, lengths=lens, m=4, freq=f.data_ptr(), n_bins=5,
             mtf=out.data_ptr(), edges=out[32:].data_ptr(), flags=iout[32:].data_ptr()):
        return lib.ol_geometric_mtf(dt, k, coords, lengths, m, freq, None, n_bins, mtf,
                                    iout.data_ptr(), edges, flags, None)

    assert call(n_bins=_capi.MTF_MAX_BINS + 1) == -1 and b"n_bins" in lib.ol_last_error()
    assert call(n_bins=0) == -1 and b"n_bins" in lib.ol_last_error()
    assert call(k=_capi.MTF_MAX_CURVES + 1) == -1 and b"n_curves" in lib.ol_last_error()
    assert call(dt=7) == -1 and b"dtype" in lib.ol_last_error()
    assert call(coords=None) == -1 and b"NULL" in lib.ol_last_error()
    assert call(lengths=None) == -1 and b"NULL" in lib.ol_last_error()
    assert call(freq=None) == -1 and b"freq" in lib.ol_last_error()
    assert call(mtf=None) == -1 and b"mtf_out" in lib.ol_last_error()
    assert call(edges=None) == -1 and b"edges_minmax_out" in lib.ol_last_error()
    assert call(flags=None) == -1 and b"flags_out" in lib.ol_last_error()
    hole = (C.c_void_p * 2)(x.data_ptr(), None)
    assert call(coords=hole) == -1 and b"coords[1] is NULL" in lib.ol_last_error()
    neg = (C.c_int64 * 2)(16, -1)
    assert call(lengths=neg) == -1 and b"negative" in lib.ol_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="n_bins"):
        geometric_mtf([x], f, n_bins=_capi.MTF_MAX_BINS + 1)


# ------------------------------------------------------------------ 6. stand-alone classes
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", M.cases(GOLD))
def test_standalone_geometric_mtf(case, dtype):
    lens = str(GOLD[f"{case}/system"])
    tracer = tr.HipRayTracer(load_system(M.SYSTEMS[lens]), DEV, dtype=dtype)
    m = GeometricMTF(tracer, **M.kwargs(GOLD, case))
    assert np.allclose(m.freq, GOLD[f"{case}/freq"], rtol=1e-12, atol=0)
    assert m.cutoff_freq == pytest.approx(float(GOLD[f"{case}/cutoff_freq"]), rel=1e-12)
    assert float(m.max_freq) == pytest.approx(float(GOLD[f"{case}/max_freq"]), rel=1e-12)
    assert np.allclose(np.broadcast_to(m.diff_limited_mtf, m.freq.shape),
                       np.broadcast_to(GOLD[f"{case}/diff_limited_mtf"], m.freq.shape),
                       rtol=0, atol=1e-12)
    want = GOLD[f"{case}/mtf"]
    assert len(m.mtf) == want.shape[0] and all(len(f) == 2 for f in m.mtf)
    got = np.array([[t.cpu().numpy(), s.cpu().numpy()] for t, s in m.mtf])
    assert got.shape == want.shape and m.mtf[0][0].dtype == torch.float64
    err = float(np.max(np.abs(got - want)))
    print(f"\n[own {'fp64' if dtype == torch.float64 else 'fp32'}] {case}: "
          f"max |stand-alone - reference| = {err:.3e}")
    tol = TOL_OWN_FP64 if dtype == torch.float64 else 3 * float(GOLD[f"{case}/fp32_spread"])
    assert err <= tol, (case, err, tol)


@pytest.mark.parametrize("case", M.fft_cases(GOLD))
def test_standalone_fft_mtf(case):
    tracer = tr.HipRayTracer(load_system(M.SYSTEMS[str(GOLD[f"{case}/system"])]), DEV,
                             dtype=torch.float64)
    mf = float(GOLD[f"{case}/max_freq_in"])
    m = FFTMTF(tracer, num_rays=int(GOLD[f"{case}/num_rays"]),
               grid_size=int(GOLD[f"{case}/grid_size"]), max_freq="cutoff" if np.isnan(mf) else mf)
    want = GOLD[f"{case}/mtf"]
    got = np.array([[t.cpu().numpy(), s.cpu().numpy()] for t, s in m.mtf])
    assert got.shape == want.shape
    # (the FFT PSF's own parity with the reference: tests/test_gpu_wavefront.py)
    assert float(np.max(np.abs(got - want))) <= 1e-9
    assert np.allclose(np.array(m.freq_tang), GOLD[f"{case}/freq_tang"], rtol=1e-9, atol=0)
    assert np.allclose(np.array(m.freq_sag), GOLD[f"{case}/freq_sag"], rtol=1e-9, atol=0)
    assert float(m.max_freq) == pytest.approx(float(GOLD[f"{case}/max_freq"]), rel=1e-9)


# ------------------------------------------------------------------ 7. the drop-in seam
class _Backend(types.ModuleType):
    _backends = {}

    @staticmethod
    def get_backend():
        return "torch"


class _Spot:
    def __init__(self, x, y):
        self.x, self.y = x, y


@pytest.mark.parametrize("precision", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", ["cooke", "dgauss", "cooke_noscale", "cooke_hex12"])
def test_seam_function_on_golden_hits(case, precision):
    """`analysis_seams._geometric_mtf_generate` called directly (no reference needed: the
    backend module it asks for its name is stood in for).  A float32 backend gets the fp64
    result of its float32 hits, cast down."""
    from optiland_amd import analysis_seams as seams

    me = types.SimpleNamespace(
        data=[[_Spot(_dev(x, precision), _dev(y, precision))] for x, y in M.hits(GOLD, case)],
        freq=_dev(GOLD[f"{case}/freq"], precision), num_points=int(GOLD[f"{case}/num_points"]),
        scale=bool(GOLD[f"{case}/scale"]), cutoff_freq=float(GOLD[f"{case}/cutoff_freq"]))
    fake = {"optiland": types.ModuleType("optiland"), "optiland.backend": _Backend("be")}
    saved = {k: sys.modules.get(k) for k in fake}
    sys.modules.update(fake)
    before = dict(seams.STATS)
    try:
        mtf, scale_factor = seams._geometric_mtf_generate(me)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert {k: sys.modules.get(k) for k in fake} == saved
    assert seams.STATS["geo_mtf"] == before["geo_mtf"] + 1
    assert seams.STATS["geo_mtf_fallback"] == before["geo_mtf_fallback"]
    want = GOLD[f"{case}/mtf"]
    assert len(mtf) == want.shape[0]
    for f, pair in enumerate(mtf):
        assert len(pair) == 2
        for a, curve in enumerate(pair):
            assert isinstance(curve, torch.Tensor) and curve.device.type == "cuda"
            assert curve.dtype == precision and curve.shape == want[f, a].shape
    got = np.array([[t.double().cpu().numpy(), s.double().cpu().numpy()] for t, s in mtf])
    if me.scale:
        assert isinstance(scale_factor, torch.Tensor) and scale_factor.dtype == precision
        assert np.allclose(scale_factor.double().cpu().numpy(), GOLD[f"{case}/diff_limited_mtf"],
                           rtol=0, atol=1e-12 if precision == torch.float64 else 1e-6)
    else:
        assert scale_factor == 1
    if precision == torch.float64:
        assert float(np.max(np.abs(got - want))) <= TOL_GIVEN
    else:
        # float32 hits are other hits (half an ulp of 25 mm is 1e-6 mm): the yardstick is the
        # NumPy sum of the SAME widened values and frequencies, to float32's rounding of a
        # curve in [0, 1]
        freq = GOLD[f"{case}/freq"].astype(np.float32).astype(np.float64)
        ratio = np.clip(freq / me.cutoff_freq, 0.0, 1.0)
        phi = np.arccos(ratio)
        scale = 2 / np.pi * (phi - np.cos(phi) * np.sin(phi)) if me.scale else None
        ref = M.numpy_geometric_mtf(
            [c.astype(np.float32).astype(np.float64) for c in M.curves(GOLD, case)], freq, scale)
        assert float(np.max(np.abs(got.reshape(ref.shape) - ref))) <= 2.0 ** -23
