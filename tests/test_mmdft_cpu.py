"""The MMDFT PSF without a GPU: the argument rules of `ol_mmdft_psf` through the product
library, the binding of a library without the entry point, the host logic of the stand-alone
`MMDFTPSF` (num_rays / image_size / pixel_pitch rules, working F/#, pad size, both ValueErrors,
the reference's parameter tables) against the reference's numbers with the product replaced by a
NumPy restatement, the drop-in seam's fall-backs, and the exact fixture's self-check."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

from optiland_amd import _capi, build, engine, load_system
from optiland_amd import tracer as tr
from optiland_amd.wavefront import MMDFTPSF
from tests import _mmdft as MM

GOLD = MM.golden()


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _capi.load()


def test_argument_validation_without_a_device(lib):
    assert _capi.has_mmdft(lib) and "ol_mmdft_psf" in _capi.EXPORTS
    pads = (C.c_double * 4)(32.0, 40.5, 48.0, 64.0)
    big = _capi.MMDFT_MAX_SIDE + 1

    # (the pointers 16 are never dereferenced: the call must fail first)
    def call(b=4, n=8, pupil=16, pad=pads, m=8, psf=16):
        return lib.ol_mmdft_psf(b, n, pupil, pad, m, psf, None, None)

    assert call(pupil=None) == -1 and b"pupil is NULL" in lib.ol_last_error()
    assert call(pad=None) == -1 and b"pad_size is NULL" in lib.ol_last_error()
    assert call(psf=None) == -1 and b"psf_out is NULL" in lib.ol_last_error()
    assert call(b=-1) == -1 and b"negative count" in lib.ol_last_error()
    for n in (0, -3, big):
        assert call(n=n) == -1 and b"n_side" in lib.ol_last_error()
    for m in (0, -3, big):
        assert call(m=m) == -1 and b"image_size" in lib.ol_last_error()
    for k, bad in enumerate((0.0, -32.0, math.nan, math.inf)):
        bad_pads = (C.c_double * 4)(32.0, 40.5, 48.0, 64.0)
        bad_pads[k] = bad
        assert call(pad=bad_pads) == -1
        assert f"pad_size[{k}]".encode() in lib.ol_last_error()
    # nothing to write: no device needed
    assert call(b=0) == 0
    assert lib.ol_mmdft_psf(0, 8, None, None, 8, None, None, None) == 0


def test_a_library_without_the_entry_point_binds_and_asks_for_a_rebuild(monkeypatch):
    from tests import _hostmath as hm
    if not hm.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    host = hm.load()          # bound through _capi.bind(); has no ol_mmdft_psf
    assert not _capi.has_mmdft(host)
    monkeypatch.setattr(_capi, "load", lambda: host)
    with pytest.raises(_capi.HipExtensionError, match="rebuild"):
        engine.mmdft_psf(np.zeros((4, 4), dtype=np.complex128), 8.0, 8)


def test_engine_refuses_bad_shapes_before_any_library():
    g = np.zeros((4, 4), dtype=np.complex128)
    with pytest.raises(ValueError, match="shape"):
        engine.mmdft_psf(np.zeros((4, 5), dtype=np.complex128), 8.0, 8)
    with pytest.raises(ValueError, match="complex"):
        engine.mmdft_psf(np.zeros((4, 4)), 8.0, 8)
    with pytest.raises(ValueError, match="pad_size"):
        engine.mmdft_psf(g, [8.0, 9.0], 8)
    with pytest.raises(ValueError, match=r"pad_size\[1\]"):
        engine.mmdft_psf(np.zeros((2, 4, 4), dtype=np.complex128), [8.0, -1.0], 8)
    with pytest.raises(ValueError, match="image_size"):
        engine.mmdft_psf(g, 8.0, 0)
    with pytest.raises(ValueError, match="image_size"):
        engine.mmdft_psf(g, 8.0, 7.5)


@pytest.fixture(params=["oracle", "kernel-source"])
def cpu_engine(monkeypatch, request):
    if request.param == "oracle":
        from tests._fake_engine import OracleEngine
        monkeypatch.setattr(tr, "_make_engine", lambda table, device: OracleEngine(table, device))
    else:
        from tests import _hostmath as hm
        if not hm.available():
            pytest.skip("hipcc (used as host C++ compiler) missing")
        cls = hm.make_engine_class()
        monkeypatch.setattr(tr, "_make_engine", lambda table, device: cls(table, device))


def _numpy_product(self, pupil, pad_size, image_size):
    out = MM.direct(pupil.detach().cpu().numpy(), pad_size, image_size)
    return torch.as_tensor(out, device=pupil.device)


def _no_product(self, pupil, pad_size, image_size):
    return torch.zeros((image_size, image_size), dtype=torch.float64)


def _tracer(system):
    return tr.HipRayTracer(load_system(MM.SYSTEMS[system]), "cpu", dtype=torch.float64)


@pytest.mark.parametrize("case", MM.cases(GOLD))
def test_standalone_host_logic_matches_the_reference(case, cpu_engine, monkeypatch):
    monkeypatch.setattr(MMDFTPSF, "_product", _numpy_product)
    psf = MMDFTPSF(_tracer(str(GOLD[f"{case}/system"])), tuple(GOLD[f"{case}/field"]),
                   float(GOLD[f"{case}/wavelength"]), **MM.kwargs(GOLD, case))
    assert psf.num_rays == int(GOLD[f"{case}/num_rays"])
    assert psf.image_size == int(GOLD[f"{case}/image_size"])
    for name, have in (("pixel_pitch", psf.pixel_pitch), ("pad_size", psf.pad_size()),
                       ("working_fno", psf.working_fno()), ("strehl", psf.strehl_ratio())):
        assert have == pytest.approx(float(GOLD[f"{case}/{name}"]), rel=1e-9, abs=1e-12), name
    assert psf.pupil.shape == GOLD[f"{case}/pupil"].shape
    assert MM.count(psf.pupil.numpy()) == int(GOLD[f"{case}/count"])
    want = GOLD[f"{case}/psf"]
    assert psf.psf.shape == want.shape
    assert np.max(np.abs(psf.psf.numpy() - want)) <= 1e-7 * np.max(want)


def test_both_value_errors(cpu_engine, monkeypatch):
    monkeypatch.setattr(MMDFTPSF, "_product", _no_product)
    with pytest.raises(ValueError, match="num_rays must be at least 32 if image_size and "
                                         "pixel_pitch are not specified."):
        MMDFTPSF(_tracer("cooke"), (0.0, 0.0), 0.55, num_rays=16)
    num_rays, image_size, pitch = GOLD["too_large/request"]
    with pytest.raises(ValueError) as err:
        MMDFTPSF(_tracer(str(GOLD["too_large/system"])), tuple(GOLD["too_large/field"]),
                 float(GOLD["too_large/wavelength"]), num_rays=int(num_rays),
                 image_size=int(image_size), pixel_pitch=float(pitch))
    assert str(err.value) == str(GOLD["too_large/error"])
    # below 32 rays is fine once a size is given (the reference's test_num_rays_below_32)
    assert MMDFTPSF(_tracer("cooke"), (0.0, 0.0), 0.55, num_rays=12, image_size=16).num_rays == 12


@pytest.mark.parametrize("table,request_of", [
    ("from_num_rays", lambda v: dict(num_rays=int(v), image_size=None)),
    ("from_pixel_pitch", lambda v: dict(num_rays=128, image_size=None, pixel_pitch=float(v))),
    ("from_image_size", lambda v: dict(num_rays=128, image_size=int(v)))])
def test_parameter_tables_of_the_reference(table, request_of, monkeypatch):
    """The reference's test_calcs_from_num_rays / _pixel_pitch / _image_size (Cooke triplet,
    (0, 0), 0.55 um), as the reference resolved them; the product itself is left out."""
    from tests._fake_engine import OracleEngine
    monkeypatch.setattr(tr, "_make_engine", lambda table, device: OracleEngine(table, device))
    monkeypatch.setattr(MMDFTPSF, "_product", _no_product)
    tracer = _tracer("cooke")
    for request, num_rays, image_size, pitch in GOLD[f"table/{table}"]:
        psf = MMDFTPSF(tracer, (0.0, 0.0), 0.55, **request_of(request))
        assert (psf.num_rays, psf.image_size) == (int(num_rays), int(image_size)), request
        assert psf.pixel_pitch == pytest.approx(float(pitch), rel=1e-9), request


# ------------------------------------------------------------------ the drop-in seam
@pytest.fixture
def reference():
    from tests import _live
    try:
        be = _live.import_reference()
    except ImportError:
        pytest.skip("reference package not present")
    yield be
    be.set_backend("numpy")


def test_seam_installs_falls_back_and_is_removed(reference, monkeypatch, tmp_path):
    from optiland.psf import mmdft as ref
    from optiland.samples.objectives import CookeTriplet

    from optiland_amd import analysis_seams as seams

    be = reference
    # (an earlier test may have left the seams on: the stock method is what disable() restores)
    was_enabled = bool(seams._ORIG)
    seams.disable()
    stock = ref.MMDFTPSF._compute_psf
    assert stock is not seams._mmdft_compute_psf
    seams.enable()
    try:
        assert "mmdft" not in seams.SKIPPED
        assert ref.MMDFTPSF._compute_psf is seams._mmdft_compute_psf
        be.set_backend("torch")
        be.set_device("cpu")
        be.set_precision("float64")
        before = dict(seams.STATS)
        psf = ref.MMDFTPSF(CookeTriplet(), (0.0, 0.0), 0.55, num_rays=32, image_size=32)
        # CPU tensors: the reference's own product
        assert seams.STATS["mmdft_fallback"] == before["mmdft_fallback"] + 1
        assert seams.STATS["mmdft"] == before["mmdft"]
        # ... and on the fixture's own pupil it gives the fixture's PSF.  (The PSF of the
        # constructor above is 5.6e-12 of the peak away from it: the torch backend's trace puts
        # 3e-10 of difference into the pupil before any product runs.)
        psf.pupil = torch.as_tensor(GOLD["cooke_00/pupil"])
        got = psf._compute_psf()
        assert seams.STATS["mmdft_fallback"] == before["mmdft_fallback"] + 2
        want = GOLD["cooke_00/psf"]
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64
        assert np.allclose(np.asarray(be.to_numpy(got)), want, rtol=0, atol=1e-12 * np.max(want))

        # on a HIP device (pretended): a subclass with its own kernels keeps its own code, and
        # a library without the entry point is declined -- each with its reason
        log = tmp_path / "seams.log"
        monkeypatch.setenv("OPTILAND_HIP_SEAM_LOG", str(log))
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)

        class Mine(ref.MMDFTPSF):
            def _compute_kernels(self):
                return super()._compute_kernels()

        mine = Mine.__new__(Mine)
        mine.__dict__.update(psf.__dict__)
        assert seams._mmdft_device(mine) is None
        assert "Mine overrides _compute_kernels" in log.read_text()
        assert seams._mmdft_device(psf) is None   # the stock class: only its CPU pupil is wrong
        assert "off the HIP device" in log.read_text().splitlines()[-1]
        monkeypatch.setattr(_capi, "has_mmdft", lambda lib: False)
        assert seams._mmdft_device(psf) is None
        assert "library without ol_mmdft_psf" in log.read_text().splitlines()[-1]
    finally:
        seams.disable()
    assert ref.MMDFTPSF._compute_psf is stock
    if was_enabled:
        seams.enable()


# ------------------------------------------------------------------ the exact fixture
def test_exact_fixture_numpy_formula_is_within_the_reference_error():
    """Self-check of tests/golden/exact_mmdft.npz: the stored NumPy-formula PSF stands within
    `REFERENCE_ERROR` of the stored exact one, and `direct` still reproduces what was stored."""
    pytest.importorskip("mpmath")
    g = MM.exact()
    for case in MM.cases(g):
        pupil, pad, m = g[f"{case}/pupil"], float(g[f"{case}/pad_size"]), int(g[f"{case}/image_size"])
        exact, stored = g[f"{case}/psf"], g[f"{case}/numpy_psf"]
        peak = float(np.max(exact))
        assert np.max(np.abs(stored - exact)) <= MM.REFERENCE_ERROR * peak, case
        assert np.max(np.abs(MM.direct(pupil, pad, m) - stored)) <= 1e-15 * peak, case
        assert float(g[f"{case}/sum_abs"]) == pytest.approx(np.abs(pupil).sum(), rel=1e-15)
        assert int(g[f"{case}/count"]) == MM.count(pupil)
        # and the exact field obeys the PSF it is stored with
        c = int(g[f"{case}/count"])
        assert np.allclose(np.abs(g[f"{case}/field"]) ** 2 * 100 / c ** 2, exact, rtol=1e-15 * 8,
                           atol=0)
