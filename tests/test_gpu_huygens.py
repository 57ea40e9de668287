"""`ol_huygens_psf` (optiland_amd/csrc/huygens.hip) on the MI355X: the reference's own
`compute()` calls (tests/golden/huygens.npz), random sums against a NumPy fp64 direct sum,
bit-reproducibility, the small-image split, the refusals, the stand-alone `HuygensPSF` and the
drop-in seam -- all without the reference package."""

import ctypes as C

import numpy as np
import pytest
import torch

from optiland_amd import _capi, load_system
from optiland_amd import tracer as tr
from optiland_amd.engine import huygens_sum
from optiland_amd.wavefront import HuygensPSF
from tests import _huygens as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = H.golden()


def _dev(v):
    return torch.as_tensor(np.asarray(v), device=DEV)


def _sum(args, **kw):
    ix, iy, iz, px, py, pz, amp, opd, wl, rp = args
    return huygens_sum(*(_dev(v) for v in (ix, iy, iz, px, py, pz, amp, opd)), float(wl),
                       float(rp), **kw)


@pytest.mark.parametrize("case", H.cases(GOLD))
def test_golden_compute_calls(case):
    for args, want in H.calls(GOLD, case):
        got = _sum(args).cpu().numpy()
        assert got.shape == want.shape
        err = np.max(np.abs(got - want)) / np.max(want)
        assert err <= 1e-10, (case, want.shape, err)


@pytest.mark.parametrize("n_image,n_pupil", [(1, 20000), (7, 20000), (32 * 32, 20000),
                                              (128 * 128, 2000)])
@pytest.mark.parametrize("complex_amp", [False, True])
def test_random_sums_match_numpy(n_image, n_pupil, complex_amp):
    args = H.random_case(n_pupil, n_image, complex_amp, seed=n_image + n_pupil)
    want = H.direct_field(*args)
    psf, field = _sum(args, want_field=True)
    field = field.cpu().numpy()
    peak = np.max(np.abs(want) ** 2)
    assert np.max(np.abs(psf.cpu().numpy() - np.abs(want) ** 2)) <= 1e-9 * peak
    assert np.max(np.abs(field - want)) <= 1e-9 * np.sqrt(peak)


def test_one_pixel_is_the_pixel_of_a_large_image():
    args = H.random_case(12000, 128 * 128, seed=3)
    big = _sum(args).cpu().numpy()
    for m in (0, 777, 128 * 128 - 1):
        one = _sum(tuple(np.asarray(a)[m:m + 1] for a in args[:3]) + args[3:]).cpu().numpy()
        assert abs(one[0] - big[m]) <= 1e-12 * np.max(big), m


@pytest.mark.parametrize("n_image", [1, 7, 128 * 128])
def test_bit_identical_from_run_to_run(n_image):
    args = H.random_case(12900, n_image, complex_amp=True, seed=5)
    a, fa = _sum(args, want_field=True)
    b, fb = _sum(args, want_field=True)
    assert torch.equal(a, b) and torch.equal(fa, fb)


def test_nan_sample_makes_every_pixel_nan_and_fp32_is_widened():
    args = list(H.random_case(500, 64, seed=7))
    want = H.direct_sum(*args)
    got32 = huygens_sum(*(_dev(np.asarray(v, dtype=np.float32)) for v in args[:8]),
                        args[8], args[9])
    assert got32.dtype == torch.float64
    args32 = [np.asarray(v, dtype=np.float32).astype(np.float64) for v in args[:8]] + args[8:]
    assert np.allclose(got32.cpu().numpy(), H.direct_sum(*args32), rtol=0,
                       atol=1e-9 * np.max(want))
    args[7] = np.array(args[7])
    args[7][123] = np.nan
    assert torch.isnan(_sum(tuple(args))).all()


def test_empty_pupil_writes_zeros_and_empty_image_is_a_no_op():
    args = H.random_case(0, 9)
    assert torch.equal(_sum(args), torch.zeros(9, dtype=torch.float64, device=DEV))
    assert _sum(H.random_case(10, 0)).numel() == 0


def test_refusals():
    lib = _capi.load()
    x = torch.zeros(4, dtype=torch.float64, device=DEV)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    pup = (C.c_void_p * 5)(*([x.data_ptr()] * 5))
    img = (C.c_void_p * 3)(*([x.data_ptr()] * 3))
    p, o = out.data_ptr(), None

    def call(n=4, pupil=pup, image=img, wl=5e-4, rp=50.0, psf=p, m=4):
        return lib.ol_huygens_psf(n, pupil, None, m, image, wl, rp, psf, o, None)

    assert call(pupil=None) == -1 and b"NULL" in lib.ol_last_error()
    assert call(image=None) == -1
    assert call(psf=None) == -1 and b"psf_out" in lib.ol_last_error()
    assert call(n=-1) == -1 and b"negative" in lib.ol_last_error()
    assert call(m=-2) == -1
    assert call(wl=0.0) == -1 and b"wavelength" in lib.ol_last_error()
    assert call(wl=-1e-3) == -1
    assert call(wl=float("nan")) == -1
    assert call(rp=0.0) == -1 and b"Rp" in lib.ol_last_error()
    hole = (C.c_void_p * 5)(*([x.data_ptr()] * 4 + [None]))
    assert call(pupil=hole) == -1 and b"pupil[4]" in lib.ol_last_error()
    assert call() == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", H.cases(GOLD))
def test_standalone_huygens_psf(case):
    system = H.SYSTEMS[str(GOLD[f"{case}/system"])]
    field = tuple(GOLD[f"{case}/field"])
    over, pitch = float(GOLD[f"{case}/oversample"]), float(GOLD[f"{case}/pixel_pitch_in"])
    tracer = tr.HipRayTracer(load_system(system), DEV, dtype=torch.float64)
    psf = HuygensPSF(tracer, field, float(GOLD[f"{case}/wavelength"]), num_rays=32,
                     image_size=32, oversample=None if np.isnan(over) else over,
                     pixel_pitch=None if np.isnan(pitch) else pitch)
    want = GOLD[f"{case}/psf"]
    got = psf.psf.cpu().numpy()
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-7 * np.max(want)
    for name, have in (("strehl", psf.strehl_ratio()), ("pixel_pitch", psf.pixel_pitch),
                       ("cx", psf.cx), ("cy", psf.cy), ("normalization", psf.normalization)):
        want_v = float(GOLD[f"{case}/{name}"])
        assert have == pytest.approx(want_v, rel=1e-9, abs=1e-12), name


@pytest.mark.parametrize("case", ["cooke_01", "dgauss_007"])
def test_seam_function_on_golden_inputs(case):
    """`analysis_seams._huygens_torch_compute` called directly (no reference needed: the
    backend module it asks for its precision is stood in for)."""
    import sys
    import types

    from optiland_amd import analysis_seams as seams

    class _Backend(types.ModuleType):
        _backends = {}

        @staticmethod
        def get_backend():
            return "torch"

        @staticmethod
        def get_complex_precision():
            return torch.complex128

    class _Self:
        device = "cuda"

    fake = {"optiland": types.ModuleType("optiland"), "optiland.backend": _Backend("be")}
    saved = {k: sys.modules.get(k) for k in fake}
    sys.modules.update(fake)
    before = seams.STATS["huygens"]
    try:
        for args, want in H.calls(GOLD, case):
            got = seams._huygens_torch_compute(_Self(), *(_dev(a) for a in args[:8]),
                                               float(args[8]), _dev(args[9]))
            assert isinstance(got, torch.Tensor) and got.device.type == "cuda"
            assert got.dtype == torch.float64 and got.shape == want.shape
            got = got.cpu().numpy()
            assert np.max(np.abs(got - want)) / np.max(want) <= 1e-10
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert seams.STATS["huygens"] == before + 2
