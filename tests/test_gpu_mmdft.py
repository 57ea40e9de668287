"""`ol_mmdft_psf` (optiland_amd/csrc/mmdft.hip) on the MI355X: the reference's recorded PSFs
(tests/golden/mmdft.npz), random pupils against the NumPy restatement of the reference's formula
at the shapes where the tiles end, batches, bit-reproducibility, the NaN rules, the refusals, the
stand-alone `MMDFTPSF` and the drop-in seam -- all without the reference package.

Tolerances (tests/_mmdft.py): against the reference's formula, the kernel's bound against the
exact transform plus twice the reference's own distance from it as measured on the CPU."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

from optiland_amd import _capi, load_system
from optiland_amd import tracer as tr
from optiland_amd.engine import mmdft_psf
from optiland_amd.wavefront import MMDFTPSF
from tests import _mmdft as MM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = MM.golden()


def _dev(v):
    return torch.as_tensor(np.asarray(v), device=DEV)


def _check_against_formula(pupil, pad, m, got, label):
    want = MM.direct(pupil, pad, m)
    tol = MM.reference_tolerance(pupil, want)
    err = np.abs(got - want)
    print(f"\n[mmdft] {label}: max |device - formula| / peak {err.max() / want.max():.3e}, "
          f"worst error / tolerance {float((err / tol).max()):.3e}")
    assert got.shape == want.shape == (m, m)
    assert np.all(err <= tol), label


@pytest.mark.parametrize("case", MM.cases(GOLD))
def test_golden_psfs_of_the_reference(case):
    pupil, pad = GOLD[f"{case}/pupil"], float(GOLD[f"{case}/pad_size"])
    want = GOLD[f"{case}/psf"]
    got = mmdft_psf(_dev(pupil), pad, want.shape[0]).cpu().numpy()
    tol = MM.reference_tolerance(pupil, want)
    err = np.abs(got - want)
    print(f"\n[mmdft golden] {case}: max |device - reference| / peak "
          f"{err.max() / want.max():.3e}, worst error / tolerance {float((err / tol).max()):.3e}")
    assert got.shape == want.shape
    assert np.all(err <= tol)


@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (17, 7), (32, 32), (33, 48), (45, 105),
                                 (64, 33), (181, 512)])
def test_random_pupils_match_the_formula(n, m):
    pupil = MM.random_pupil(n, seed=1000 * n + m)
    pad = max(n, m) + 0.65 if (n, m) != (1, 1) else 1.0
    psf, field = mmdft_psf(_dev(pupil), pad, m, want_field=True)
    assert psf.dtype == torch.float64 and field.dtype == torch.complex128
    _check_against_formula(pupil, pad, m, psf.cpu().numpy(), f"N {n} M {m} pad {pad}")
    # the field that was written is the field the PSF was taken of
    f = field.cpu().numpy()
    c = MM.count(pupil)
    assert np.allclose((f.real ** 2 + f.imag ** 2) * 100 / c ** 2, psf.cpu().numpy(),
                       rtol=4 * MM.EPS, atol=0)


def test_batch_equals_single_calls_bit_for_bit():
    pupils = MM.random_pupil(45, seed=11, batch=3)
    pads = [105.65036602741444, 128.0, 110.25]
    psf, field = mmdft_psf(_dev(pupils), pads, 105, want_field=True)
    assert psf.shape == (3, 105, 105) and field.shape == (3, 105, 105)
    for k in range(3):
        one, one_field = mmdft_psf(_dev(pupils[k]), pads[k], 105, want_field=True)
        assert torch.equal(one, psf[k]) and torch.equal(one_field, field[k]), k
        _check_against_formula(pupils[k], pads[k], 105, one.cpu().numpy(), f"batch member {k}")


def test_more_pupils_than_one_launch_takes():
    """40 pupils: two slices of the entry point's 32."""
    pupils = MM.random_pupil(9, seed=12, batch=40)
    pads = [16.0 + 0.125 * k for k in range(40)]
    psf = mmdft_psf(_dev(pupils), pads, 16)
    for k in (0, 31, 32, 39):
        assert torch.equal(psf[k], mmdft_psf(_dev(pupils[k]), pads[k], 16)), k


@pytest.mark.parametrize("n,m", [(17, 7), (64, 130)])
def test_bit_identical_from_run_to_run(n, m):
    pupil = _dev(MM.random_pupil(n, seed=5))
    a, fa = mmdft_psf(pupil, m + 0.5, m, want_field=True)
    b, fb = mmdft_psf(pupil, m + 0.5, m, want_field=True)
    assert torch.equal(a, b) and torch.equal(fa, fb)


def test_empty_pupil_and_nan_cell_give_nan_everywhere():
    zero = torch.zeros((33, 33), dtype=torch.complex128, device=DEV)
    assert torch.isnan(mmdft_psf(zero, 70.5, 70)).all()
    pupil = MM.random_pupil(33, seed=7, batch=2)
    pupil[1, 20, 13] = complex(np.nan, 0.0)
    psf = mmdft_psf(_dev(pupil), [70.5, 70.5], 70)
    assert torch.isnan(psf[1]).all()
    # ... of that pupil alone
    assert torch.equal(psf[0], mmdft_psf(_dev(pupil[0]), 70.5, 70))


def test_complex64_is_widened():
    pupil = MM.random_pupil(33, seed=8).astype(np.complex64)
    got = mmdft_psf(_dev(pupil), 48.0, 48)
    assert got.dtype == torch.float64
    assert torch.equal(got, mmdft_psf(_dev(pupil.astype(np.complex128)), 48.0, 48))


def test_refusals():
    lib = _capi.load()
    g = torch.zeros((4, 8, 8), dtype=torch.complex128, device=DEV)
    out = torch.zeros((4, 8, 8), dtype=torch.float64, device=DEV)
    pads = (C.c_double * 4)(8.0, 9.5, 12.0, 16.0)
    big = _capi.MMDFT_MAX_SIDE + 1

    def call(b=4, n=8, pupil=g.data_ptr(), pad=pads, m=8, psf=out.data_ptr()):
        return lib.ol_mmdft_psf(b, n, pupil, pad, m, psf, None, None)

    assert call(pupil=None) == -1 and b"pupil is NULL" in lib.ol_last_error()
    assert call(pad=None) == -1 and b"pad_size is NULL" in lib.ol_last_error()
    assert call(psf=None) == -1 and b"psf_out is NULL" in lib.ol_last_error()
    assert call(b=-1) == -1 and b"negative" in lib.ol_last_error()
    assert call(n=0) == -1 and call(n=big) == -1 and b"n_side" in lib.ol_last_error()
    assert call(m=0) == -1 and call(m=big) == -1 and b"image_size" in lib.ol_last_error()
    for bad in (0.0, -1.0, math.nan, math.inf):
        bad_pads = (C.c_double * 4)(8.0, 9.5, bad, 16.0)
        assert call(pad=bad_pads) == -1 and b"pad_size[2]" in lib.ol_last_error()
    assert call(b=0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()   # (four empty pupils: 0 * 100 / 0)


@pytest.mark.parametrize("case", MM.cases(GOLD))
def test_standalone_mmdft_psf(case):
    tracer = tr.HipRayTracer(load_system(MM.SYSTEMS[str(GOLD[f"{case}/system"])]), DEV,
                             dtype=torch.float64)
    psf = MMDFTPSF(tracer, tuple(GOLD[f"{case}/field"]), float(GOLD[f"{case}/wavelength"]),
                   **MM.kwargs(GOLD, case))
    assert psf.num_rays == int(GOLD[f"{case}/num_rays"])
    assert psf.image_size == int(GOLD[f"{case}/image_size"])
    for name, have in (("pixel_pitch", psf.pixel_pitch), ("pad_size", psf.pad_size()),
                       ("working_fno", psf.working_fno()), ("strehl", psf.strehl_ratio())):
        assert have == pytest.approx(float(GOLD[f"{case}/{name}"]), rel=1e-9, abs=1e-12), name
    assert psf.pupil.is_cuda and psf.psf.is_cuda
    assert MM.count(psf.pupil.cpu().numpy()) == int(GOLD[f"{case}/count"])
    want = GOLD[f"{case}/psf"]
    got = psf.psf.cpu().numpy()
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-7 * np.max(want)


@pytest.mark.parametrize("precision", [torch.complex128, torch.complex64])
@pytest.mark.parametrize("case", ["cooke_01_m48", "dgauss_007_pitch"])
def test_seam_function_on_golden_inputs(case, precision):
    """`analysis_seams._mmdft_compute_psf` called directly (no reference needed: the backend
    module it asks for its precision, and the object it is a method of, are stood in for)."""
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
            return precision

    class _Wavelength:
        value = float(GOLD[f"{case}/wavelength"])

    class _Self:
        _compute_psf = seams._mmdft_compute_psf
        wavelengths = [_Wavelength]
        pupil = _dev(GOLD[f"{case}/pupil"])
        num_rays = int(GOLD[f"{case}/num_rays"])
        image_size = int(GOLD[f"{case}/image_size"])
        pixel_pitch = float(GOLD[f"{case}/pixel_pitch"])

        def _compute_kernels(self):
            raise AssertionError("the seam must not build the reference's kernels")

        def _get_normalization(self):
            raise AssertionError("the seam must not call the reference's normalisation")

        def _get_working_FNO(self):
            return float(GOLD[f"{case}/working_fno"])

    fake = {"optiland": types.ModuleType("optiland"), "optiland.backend": _Backend("be")}
    saved = {k: sys.modules.get(k) for k in fake}
    sys.modules.update(fake)
    before = seams.STATS["mmdft"]
    try:
        me = _Self()
        got = me._compute_psf()
        me.image_size = 4 * me.image_size     # beyond the pad size: the reference's ValueError
        with pytest.raises(ValueError, match="Supplied image_size of .* not less than or equal "
                                             "to calculated pad size of"):
            me._compute_psf()
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert seams.STATS["mmdft"] == before + 1
    want = GOLD[f"{case}/psf"]
    real = torch.float32 if precision == torch.complex64 else torch.float64
    assert isinstance(got, torch.Tensor) and got.device.type == "cuda"
    assert got.dtype == real and got.shape == want.shape
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    if real == torch.float64:
        assert np.all(err <= MM.reference_tolerance(GOLD[f"{case}/pupil"], want))
    else:   # the fp64 result rounded to float32 once
        assert np.all(err <= 2.0 ** -24 * want + MM.reference_tolerance(GOLD[f"{case}/pupil"], want))
