"""The geometric MTF without a GPU: the argument rules of `ol_geometric_mtf` and of
`engine.geometric_mtf` (checked before any device is touched), the binding of a library
without the entry point, the host logic of the stand-alone `GeometricMTF` / `FFTMTF`
(wavelength, paraxial F/#, cutoff, frequencies, scale factor, curve order) against the
reference's numbers with the device transform replaced by a NumPy stand-in, and the drop-in
seam's installation and fall-backs."""

import ctypes as C

import numpy as np
import pytest
import torch

from optiland_amd import _capi, build, engine, load_system
from optiland_amd import mtf as mtf_mod
from optiland_amd import tracer as tr
from optiland_amd.mtf import FFTMTF, GeometricMTF
from tests import _geometric_mtf as M

GOLD = M.golden()


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _capi.load()


def test_argument_validation_without_a_device(lib):
    assert _capi.has_geometric_mtf(lib) and "ol_geometric_mtf" in _capi.EXPORTS
    ptrs = (C.c_void_p * 2)(16, 16)      # never dereferenced: the call must fail first
    lens = (C.c_int64 * 2)(4, 4)

    def call(dt=_capi.F64, k=2, coords=ptrs, lengths=lens, m=4, freq=16, n_bins=5, mtf=16,
             edges=16, flags=16):
        return lib.ol_geometric_mtf(dt, k, coords, lengths, m, freq, None, n_bins, mtf, None,
                                    edges, flags, None)

    assert call(dt=2) == -1 and b"dtype" in lib.ol_last_error()
    assert call(k=-1) == -1 and b"n_curves" in lib.ol_last_error()
    assert call(k=_capi.MTF_MAX_CURVES + 1) == -1 and b"n_curves" in lib.ol_last_error()
    assert call(m=-1) == -1 and b"negative count" in lib.ol_last_error()
    for n_bins in (0, -3, _capi.MTF_MAX_BINS + 1):
        assert call(n_bins=n_bins) == -1 and b"n_bins" in lib.ol_last_error()
    assert call(coords=None) == -1 and b"NULL argument" in lib.ol_last_error()
    assert call(lengths=None) == -1 and b"NULL argument" in lib.ol_last_error()
    assert call(edges=None) == -1 and b"edges_minmax_out" in lib.ol_last_error()
    assert call(flags=None) == -1 and b"flags_out" in lib.ol_last_error()
    assert call(freq=None) == -1 and b"freq" in lib.ol_last_error()
    assert call(mtf=None) == -1 and b"mtf_out" in lib.ol_last_error()
    hole = (C.c_void_p * 2)(16, None)
    assert call(coords=hole) == -1 and b"coords[1] is NULL" in lib.ol_last_error()
    assert call(lengths=(C.c_int64 * 2)(4, -4)) == -1 and b"negative count" in lib.ol_last_error()
    assert call(lengths=(C.c_int64 * 2)(4, 2 ** 31)) == -1 and b"int32" in lib.ol_last_error()
    # nothing to do: no device needed
    assert call(k=0, coords=None, lengths=None) == 0
    assert _capi.MTF_MAX_BINS >= 4097


def test_engine_checks_its_arguments_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(engine, "_require_gpu", no_device)
    monkeypatch.setattr(_capi, "load", no_device)
    x, f = np.zeros(5), np.linspace(0.0, 1.0, 4)
    with pytest.raises(ValueError, match="no curve"):
        engine.geometric_mtf([], f)
    with pytest.raises(ValueError, match="one-dimensional"):
        engine.geometric_mtf([np.zeros((2, 3))], f)
    with pytest.raises(ValueError, match="dimensions"):
        engine.geometric_mtf(np.zeros((2, 3, 4)), f)
    with pytest.raises(ValueError, match="floating point"):
        engine.geometric_mtf([torch.zeros(3, dtype=torch.int64)], f)
    with pytest.raises(ValueError, match="freq"):
        engine.geometric_mtf([x], np.zeros((2, 2)))
    with pytest.raises(ValueError, match="freq"):
        engine.geometric_mtf([x], np.zeros(0))
    with pytest.raises(ValueError, match="scale"):
        engine.geometric_mtf([x], f, scale=np.ones(3))
    for n_bins in (0, _capi.MTF_MAX_BINS + 1, 2.5):
        with pytest.raises(ValueError, match="n_bins"):
            engine.geometric_mtf([x], f, n_bins=n_bins)
    curves, num_points, n_bins = engine._mtf_arguments(np.zeros((3, 7)), f, np.ones(4), None)
    assert len(curves) == 3 and num_points == 4 and n_bins == 5


def test_a_library_without_the_entry_point_binds_and_asks_for_a_rebuild(monkeypatch):
    from tests import _hostmath as hm
    if not hm.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    host = hm.load()          # bound through _capi.bind(); has no ol_geometric_mtf
    assert not _capi.has_geometric_mtf(host)
    monkeypatch.setattr(_capi, "load", lambda: host)
    with pytest.raises(_capi.HipExtensionError, match="rebuild"):
        engine.geometric_mtf([np.zeros(3)], np.linspace(0.0, 1.0, 4))


# ------------------------------------------------------------------ stand-alone host logic
@pytest.fixture
def cpu_engine(monkeypatch):
    from tests._fake_engine import OracleEngine
    monkeypatch.setattr(tr, "_make_engine", lambda table, device: OracleEngine(table, device))


def _numpy_transform(self, curves, scale):
    out = M.numpy_geometric_mtf([c.detach().cpu().numpy() for c in curves], self.freq, scale,
                                self.num_points + 1)
    return torch.as_tensor(out)


@pytest.mark.parametrize("case", M.cases(GOLD))
def test_standalone_host_logic_matches_the_reference(case, cpu_engine, monkeypatch):
    monkeypatch.setattr(GeometricMTF, "_transform", _numpy_transform)
    lens = str(GOLD[f"{case}/system"])
    tracer = tr.HipRayTracer(load_system(M.SYSTEMS[lens]), "cpu", dtype=torch.float64)
    m = GeometricMTF(tracer, **M.kwargs(GOLD, case))
    assert m.wavelength == float(GOLD[f"{case}/wavelength"])
    assert np.allclose(np.array(m.fields), GOLD[f"{case}/fields"], rtol=0, atol=1e-15)
    assert m.cutoff_freq == pytest.approx(float(GOLD[f"{case}/cutoff_freq"]), rel=1e-12)
    assert float(m.max_freq) == pytest.approx(float(GOLD[f"{case}/max_freq"]), rel=1e-12)
    assert np.allclose(m.freq, GOLD[f"{case}/freq"], rtol=1e-12, atol=0)
    assert np.allclose(np.broadcast_to(m.diff_limited_mtf, m.freq.shape),
                       np.broadcast_to(GOLD[f"{case}/diff_limited_mtf"], m.freq.shape),
                       rtol=0, atol=1e-12)
    # the hits are the reference's (the oracle's fp64 trace), field by field, in its order
    for (x, y), (gx, gy) in zip(m.data, M.hits(GOLD, case)):
        assert x.shape == gx.shape
        assert np.allclose(x.numpy(), gx, rtol=0, atol=1e-9)
        assert np.allclose(y.numpy(), gy, rtol=0, atol=1e-9)
    want = GOLD[f"{case}/mtf"]
    got = np.array([[t.numpy(), s.numpy()] for t, s in m.mtf])
    assert got.shape == want.shape
    # (a hit may cross a bin edge between two fp64 traces: the fixture's own 1e-9 mm spread
    # is 4.7e-8 / 2.9e-8; tangential = y and sagittal = x, swapped, would be off by ~0.1)
    assert float(np.max(np.abs(got - want))) <= 1e-6


def test_paraxial_fno_and_scale_factor():
    for case in ("cooke", "dgauss"):
        table = load_system(M.SYSTEMS[case])
        cutoff = 1 / (float(GOLD[f"{case}/wavelength"]) * 1e-3 * mtf_mod.paraxial_fno(table))
        assert cutoff == pytest.approx(float(GOLD[f"{case}/cutoff_freq"]), rel=1e-12)
        scale = mtf_mod.diffraction_limited_scale(GOLD[f"{case}/freq"], cutoff)
        assert np.allclose(scale, GOLD[f"{case}/diff_limited_mtf"], rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="primary"):
        mtf_mod._resolve_wavelength(table, "all")
    with pytest.raises(TypeError):
        mtf_mod._resolve_wavelength(table, [0.55])
    with pytest.raises(ValueError, match="all"):
        mtf_mod._resolve_fields(table, "some")


def test_fft_mtf_refuses_a_polarised_system():
    table = load_system("cooke_generic")
    table.polarization = {"is_polarized": True}
    tracer = type("T", (), {"table": table})()
    with pytest.raises(NotImplementedError, match="VectorialFFTMTF"):
        FFTMTF(tracer)


@pytest.mark.parametrize("case", M.fft_cases(GOLD))
def test_fft_mtf_host_logic_matches_the_reference(case, cpu_engine):
    tracer = tr.HipRayTracer(load_system(M.SYSTEMS[str(GOLD[f"{case}/system"])]), "cpu",
                             dtype=torch.float64)
    mf = float(GOLD[f"{case}/max_freq_in"])
    m = FFTMTF(tracer, num_rays=int(GOLD[f"{case}/num_rays"]),
               grid_size=int(GOLD[f"{case}/grid_size"]), max_freq="cutoff" if np.isnan(mf) else mf)
    want = GOLD[f"{case}/mtf"]
    got = np.array([[t.numpy(), s.numpy()] for t, s in m.mtf])
    assert got.shape == want.shape
    assert float(np.max(np.abs(got - want))) <= 1e-9
    assert np.allclose(np.array(m.FNO), GOLD[f"{case}/FNO"], rtol=1e-9, atol=0)
    assert np.allclose(np.array(m.freq_tang), GOLD[f"{case}/freq_tang"], rtol=1e-9, atol=0)
    assert np.allclose(np.array(m.freq_sag), GOLD[f"{case}/freq_sag"], rtol=1e-9, atol=0)
    assert float(m.max_freq) == pytest.approx(float(GOLD[f"{case}/max_freq"]), rel=1e-9)
    assert m.freq is m.freq_tang


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
    from optiland.mtf import geometric as geo
    from optiland.samples.objectives import CookeTriplet

    from optiland_amd import analysis_seams as seams

    be = reference
    # (an earlier test may have left the seams on: the stock method is what disable() restores)
    was_enabled = bool(seams._ORIG)
    seams.disable()
    stock = geo.GeometricMTF._generate_mtf_data
    assert stock is not seams._geometric_mtf_generate
    seams.enable()
    log = tmp_path / "seams.log"
    monkeypatch.setenv("OPTILAND_HIP_SEAM_LOG", str(log))
    try:
        assert "geo_mtf" not in seams.SKIPPED
        assert geo.GeometricMTF._generate_mtf_data is seams._geometric_mtf_generate
        before = dict(seams.STATS)
        # the NumPy backend: the reference's own method, its own numbers
        m = geo.GeometricMTF(CookeTriplet(), distribution="hexapolar", num_rays=12)
        assert seams.STATS["geo_mtf_fallback"] == before["geo_mtf_fallback"] + 1
        assert seams.STATS["geo_mtf"] == before["geo_mtf"]
        got = np.array([[np.asarray(t), np.asarray(s)] for t, s in m.mtf])
        assert np.array_equal(got, GOLD["cooke_hex12/mtf"])
        assert "geo_mtf: not the torch backend" in log.read_text()
        # the torch backend on the CPU: declined as well (hits off the HIP device)
        be.set_backend("torch")
        be.set_device("cpu")
        be.set_precision("float64")
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        m = geo.GeometricMTF(CookeTriplet(), distribution="hexapolar", num_rays=12)
        assert seams.STATS["geo_mtf_fallback"] == before["geo_mtf_fallback"] + 2
        assert seams.STATS["geo_mtf"] == before["geo_mtf"]
        assert "off the HIP device" in log.read_text()
        assert len(m.mtf) == 3
    finally:
        seams.disable()
    assert geo.GeometricMTF._generate_mtf_data is stock
    if was_enabled:
        seams.enable()
