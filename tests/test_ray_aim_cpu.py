"""Iterative ray aiming without a GPU: the kernel's own source (csrc/ray_aim_device.h) compiled
for the host as a stand-alone program (tests/hostaim), plain and under AddressSanitizer +
UndefinedBehaviorSanitizer, against the reference's recorded solves; the argument rules of
`ol_aim_rays`; a library without the entry point; the engine's shape checks; the reference's two
ValueErrors from the status bits; the drop-in seam's installation and its fall-backs."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from optiland_amd import _capi, build, engine, load_system
from optiland_amd import tracer as tr
from tests import _ray_aim as RA

CASES = RA.cases()
# the paraxial launch state is a start the solve converges from (the robust lenses off axis need
# the robust aimer's continuation: from the paraxial state their first error is NaN)
PARAXIAL_OK = [c for c in CASES if c.startswith(("wa100", "relay")) or c.endswith("h00")]


# ------------------------------------------------------------------ the kernel's source, on the host
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def hostaim(request):
    b = RA._builder()
    if not b.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return b.build(sanitize=request.param == "sanitized")


def _run(exe, mode, path):
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{mode}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def host_system():
    """The host build of the trace kernels behind the C ABI (tests/hostmath): an independent
    re-trace of what the solve returns."""
    from tests import _hostmath as hm
    if not hm.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    made = {}

    def get(system):
        if system not in made:
            made[system] = hm.HostMathSystem(RA.table(system))
        return made[system]
    yield get
    for s in made.values():
        s.close()


def _retrace(host_system, c, solved):
    """Stop-plane (x, y) of the launch states `solved`, by `ol_trace_ex` over [first, stop]."""
    n = solved.shape[1]
    rays = [np.ascontiguousarray(p) for p in solved] + [np.ones(n), np.zeros(n)]
    _rec, status = host_system(c["system"]).trace(rays, 0, record=False, first=c["first"],
                                                  last=c["stop"], write_rays=True)
    assert status & ~0x20 == 0
    return RA.stop_local(c["table"], c["stop"], rays[0], rays[1], rays[2])[:2]


@pytest.mark.parametrize("name", CASES)
def test_host_solve_from_the_recorded_guess(name, hostaim, host_system, tmp_path):
    c = RA.case(name)
    path = tmp_path / "case.bin"
    RA.write_case(path, c, use_guess=True)
    solved, updates, bits, status = RA.parse_solution(_run(hostaim, "solve", path))
    assert status == 0 and not bits.any()
    err = np.max(np.abs(solved - c["solved"]), axis=0)
    print(f"{name}: max |launch - reference| = {err.max():.3e} (bound {RA.launch_bound(c).min():.3e}), "
          f"updates max {updates.max()} (reference passes {c['passes']})")
    assert np.all(err <= RA.launch_bound(c))
    # the contract, by an independent re-trace: within tol of the target on the stop plane
    lx, ly = _retrace(host_system, c, solved)
    tx, ty = c["pupil"][0] * c["r_stop"], c["pupil"][1] * c["r_stop"]
    miss = np.hypot(lx - tx, ly - ty)
    assert np.all(miss <= c["tol"] + RA.contract_slack(c, lx, ly)), miss.max()
    # same arithmetic, same step order: the counts are the reference's
    assert updates.max() == c["passes"]
    assert np.array_equal(updates, c["updates"])


@pytest.mark.parametrize("name", PARAXIAL_OK)
def test_host_solve_generating_the_paraxial_start(name, hostaim, tmp_path):
    c = RA.case(name)
    assert np.array_equal(c["guess"], c["paraxial"])
    path = tmp_path / "case.bin"
    RA.write_case(path, c, use_guess=False)
    solved, updates, bits, status = RA.parse_solution(_run(hostaim, "solve", path))
    assert status == 0
    assert np.all(np.max(np.abs(solved - c["solved"]), axis=0) <= RA.launch_bound(c))
    assert updates.max() == c["passes"]


def test_host_status_bits_and_edge_counts(hostaim, tmp_path):
    c = RA.case("wa100_h10")
    path = tmp_path / "case.bin"
    # one step is not enough at the edge of the field: a status bit, not a fault
    RA.write_case(path, c, use_guess=True, max_iter=1)
    _s, updates, bits, status = RA.parse_solution(_run(hostaim, "solve", path))
    assert status == _capi.AIM_NOT_CONVERGED and updates.max() == 1
    # no step at all: the start comes back
    RA.write_case(path, c, use_guess=True, max_iter=0)
    solved, updates, bits, status = RA.parse_solution(_run(hostaim, "solve", path))
    assert np.array_equal(solved, c["guess"]) and not updates.any()
    assert status == _capi.AIM_NOT_CONVERGED
    # one NaN ray in the guess: its bits alone, the others solve as before
    guess = c["guess"].copy()
    guess[1, 5] = np.nan
    RA.write_case(path, c, use_guess=True, guess=guess)
    solved, updates, bits, status = RA.parse_solution(_run(hostaim, "solve", path))
    assert status == _capi.AIM_NAN_GUESS | _capi.AIM_NOT_CONVERGED
    assert bits[5] == status and not np.delete(bits, 5).any()
    keep = np.arange(solved.shape[1]) != 5
    assert np.all(np.max(np.abs(solved - c["solved"]), axis=0)[keep] <= RA.launch_bound(c)[keep])
    # the robust lens from the paraxial state: NaN in the first error
    c = RA.case("wa170_h10")
    RA.write_case(path, c, use_guess=False)
    _s, _u, _b, status = RA.parse_solution(_run(hostaim, "solve", path))
    assert status & _capi.AIM_NAN_GUESS
    # n = 1 and n = 0
    c = RA.case("relay_h07")
    RA.write_case(path, c, use_guess=True, n=1)
    solved, _u, _b, status = RA.parse_solution(_run(hostaim, "solve", path))
    assert status == 0 and solved.shape == (6, 1)
    assert np.all(np.abs(solved[:, 0] - c["solved"][:, 0]) <= RA.launch_bound(c)[0])
    RA.write_case(path, c, use_guess=True, n=0)
    assert _run(hostaim, "solve", path).split() == ["status", "0"]


# ------------------------------------------------------------------ the C API's argument rules
def test_argument_rules_on_a_host_system(hostaim, tmp_path):
    c = RA.case("wa100_h07")
    path = tmp_path / "case.bin"
    RA.write_case(path, c, use_guess=True)
    got = {}
    for line in _run(hostaim, "validate", path).splitlines():
        what, rest = line.split(": ", 1)
        code, text = rest.split(" ", 1)
        got[what] = (int(code), text)
    for ok in ("good", "good guess", "empty", "max_iter 0"):
        assert got[ok] == (0, "ok"), ok
    for what, text in (("null system", "system is NULL"), ("null params", "params is NULL"),
                       ("null inputs", "px, py are required"), ("null py", "px, py are required"),
                       ("hx without hy", "given together"), ("null status", "status is NULL"),
                       ("null out", "out is NULL"), ("null out plane", "out[3] is NULL"),
                       ("null guess plane", "guess[1] is NULL"), ("negative count", "negative"),
                       ("wavelength", "wavelength index 1 outside [0, 1)"),
                       ("stop past the table", "surface range"), ("negative first", "surface range"),
                       ("first past stop", "surface range"), ("max_iter -1", "max_iter -1"),
                       ("max_iter 1001", "max_iter 1001 outside [0, 1000]"),
                       ("tol negative", "tol"), ("tol nan", "tol"), ("tol inf", "tol"),
                       ("r_stop nan", "NaN")):
        assert got[what][0] == -1 and text in got[what][1], (what, got[what])


def test_argument_rules_without_a_device():
    build.build_library()
    lib = _capi.load()
    assert _capi.has_aim_rays(lib) and "ol_aim_rays" in _capi.EXPORTS
    assert C.sizeof(_capi.AimParams) == 32 + C.sizeof(_capi.RaygenParams)
    p, inp = _capi.AimParams(1.0, 1.0, 1e-6, 10, 1), _capi.RaygenInputs()
    out = (C.c_void_p * 6)(*[16] * 6)   # (never dereferenced: the call must fail first)
    rc = lib.ol_aim_rays(None, 1, 0, 1, 2, C.byref(p), C.byref(inp), None, out, None, 16, None)
    assert rc == -1 and b"system is NULL" in lib.ol_last_error()


def test_reference_newton_range_is_refused(hostaim, tmp_path):
    """A range with an OL_SURF_REFERENCE_NEWTON surface: a batch-global rule has no per-ray form."""
    from optiland_amd import system as S
    flagged = S.SystemTable.from_json(load_system("rc_asphere").to_json())
    k = int(np.nonzero(flagged.surfaces["geom_kind"] == S.GEOM_EVEN_ASPHERE)[0][0])
    flagged.surfaces["flags"][k] |= S.SURF_REFERENCE_NEWTON
    assert flagged.reference_newton_surfaces(1, k) == [k]
    c = dict(table=flagged, pupil=np.zeros((2, 1)), guess=np.zeros((6, 1)), first=1, stop=k,
             max_iter=10, infinite=True, r_stop=1.0, jacobian=1.0, tol=1e-6, hy=0.0)
    path = tmp_path / "case.bin"
    RA.write_case(path, c, use_guess=True)
    lines = _run(hostaim, "validate", path).splitlines()
    assert lines[0].startswith(f"good: -2 ol_aim_rays: surface {k} carries OL_SURF_REFERENCE_NEWTON")
    # ... and in front of that surface the range is an ordinary one
    c["stop"] = k - 1
    RA.write_case(path, c, use_guess=True)
    assert _run(hostaim, "validate", path).splitlines()[0] == "good: 0 ok"


# ------------------------------------------------------------------ a library without the symbol
def _host_engine(system="wa100"):
    from tests import _hostmath as hm
    if not hm.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return hm.make_engine_class()(RA.table(system))


def _call(eng, c, **over):
    kw = dict(first=c["first"], stop=c["stop"], stop_radius=c["r_stop"], jacobian=c["jacobian"],
              infinite=c["infinite"], tol=c["tol"], max_iter=c["max_iter"],
              guess=[torch.as_tensor(p) for p in c["guess"]])
    px, py = (torch.as_tensor(p) for p in c["pupil"])
    kw.update(over)
    px, py = kw.pop("px", px), kw.pop("py", py)
    return eng.aim_rays(px, py, 0, **kw)


def test_a_library_without_the_entry_point_binds_and_asks_for_a_rebuild():
    eng = _host_engine()       # bound through _capi.bind(); the harness has no ol_aim_rays
    assert not _capi.has_aim_rays(eng.lib) and not eng.can_aim_rays()
    with pytest.raises(_capi.HipExtensionError, match="rebuild"):
        _call(eng, RA.case("wa100_h07"))


def test_engine_refuses_bad_shapes_before_any_library():
    eng = _host_engine()
    c = RA.case("wa100_h07")
    n = c["pupil"].shape[1]
    good = [torch.as_tensor(p) for p in c["guess"]]
    for over, text in (
            (dict(px=torch.zeros(n, dtype=torch.float32)), "px must be a 1-D float64"),
            (dict(px=torch.zeros((n, 1), dtype=torch.float64)), "px must be a 1-D float64"),
            (dict(px=np.zeros(n)), "px must be a 1-D float64"),
            (dict(py=torch.zeros(n + 1, dtype=torch.float64)), "py has"),
            (dict(guess=good[:5]), "six planes"),
            (dict(guess=good[:5] + [good[5][:-1]]), "guess N has"),
            (dict(guess=good[:5] + [good[5].float()]), "guess N must be"),
            (dict(guess=None), "either a guess"),
            (dict(field=(0.0, 0.7)), "either a guess"),
            (dict(guess=None, field=(0.0, torch.zeros(n, dtype=torch.float64))), "hx and hy"),
            (dict(guess=None, field=(0.0, 0.7), vig=(1.0,)), "vig is"),
            (dict(max_iter=-1), "max_iter"), (dict(max_iter=1001), "max_iter"),
            (dict(max_iter=2.5), "max_iter"), (dict(max_iter=True), "max_iter"),
            (dict(tol=-1e-9), "tol"), (dict(tol=float("nan")), "tol"),
            (dict(tol=float("inf")), "tol"), (dict(stop_radius=float("nan")), "NaN"),
            (dict(jacobian=float("nan")), "NaN"),
            (dict(stop=eng.num_surfaces), "surface range"), (dict(first=-1), "surface range"),
            (dict(first=c["stop"] + 1), "surface range")):
        with pytest.raises(ValueError, match=text):
            _call(eng, c, **over)


def test_both_value_errors_from_the_status_bits():
    raise_for = engine.HipSystem.raise_for_aim_status
    raise_for(0)
    raise_for(0x3f)    # the trace's own bits are not the aimer's
    with pytest.raises(ValueError) as err:
        raise_for(_capi.AIM_NAN_GUESS)
    assert str(err.value) == ("Initial ray aiming guess produced NaNs. "
                              "Consider using the 'robust' method instead.")
    with pytest.raises(ValueError) as err:
        raise_for(_capi.AIM_NOT_CONVERGED)
    assert str(err.value) == "Iterative aimer failed to converge."
    with pytest.raises(ValueError, match="produced NaNs"):   # the reference checks NaN first
        raise_for(_capi.AIM_NAN_GUESS | _capi.AIM_NOT_CONVERGED)
    # ... and they are the reference's texts, where its source is at hand
    from tests import _live
    root = _live.reference_root()
    if root is not None:
        with open(os.path.join(root, "optiland", "rays", "ray_aiming", "iterative.py")) as f:
            src = f.read()
        first, second = engine.AIM_NAN_GUESS_TEXT.split(". ", 1)   # (two literals over two lines)
        assert f'"{first}. "' in src and f'"{second}"' in src
        assert f'"{engine.AIM_NOT_CONVERGED_TEXT}"' in src


def test_standalone_tracer_entry_and_set_aiming():
    from tests._fake_engine import OracleEngine
    t = tr.HipRayTracer(RA.table("wa100"), "cpu", dtype=torch.float64,
                        engine=OracleEngine(RA.table("wa100"), "cpu"))
    with pytest.raises(NotImplementedError):
        t.set_aiming("iterative")
    with pytest.raises(NotImplementedError):
        t.set_aiming("robust")
    t.set_aiming("paraxial")
    c = RA.case("wa100_h07")
    with pytest.raises(NotImplementedError, match="ol_aim_rays"):   # an engine without it
        t.aim_rays(0.0, 0.7, c["pupil"][0], c["pupil"][1], c["wavelength"],
                   stop_radius=c["r_stop"], jacobian=c["jacobian"])
    # the stop comes from the packed table; a table written before it was packed says so
    assert RA.table("wa100").stop_index == c["stop"]
    old = load_system("double_gauss")
    if old.stop_index is None:
        t2 = tr.HipRayTracer(old, "cpu", dtype=torch.float64, engine=_host_engine())
        with pytest.raises(ValueError, match="stop"):
            t2.aim_rays(0.0, 0.7, c["pupil"][0], c["pupil"][1], 0.5876, stop_radius=1.0,
                        jacobian=1.0)
    # through the engine class on the host library: shapes pass, the library has no entry point
    t3 = tr.HipRayTracer(RA.table("wa100"), "cpu", dtype=torch.float64, engine=_host_engine())
    with pytest.raises(_capi.HipExtensionError, match="rebuild"):
        t3.aim_rays(0.0, 0.7, c["pupil"][0], c["pupil"][1], c["wavelength"],
                    stop_radius=c["r_stop"], jacobian=c["jacobian"])


def test_stop_index_survives_the_json_round_trip():
    from optiland_amd.system import SystemTable
    t = RA.table("relay")
    assert t.stop_index == 3
    assert SystemTable.from_json(t.to_json()).stop_index == 3
    t2 = SystemTable.from_json(t.to_json())
    t2.stop_index = None
    assert "stop_index" not in t2.to_json()


# ------------------------------------------------------------------ the drop-in seam
from tests.test_reference_integration import REF, hip_on_cpu, ref  # noqa: E402,F401 (fixtures)

needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "optiland")),
                                     reason="reference package not present")


@needs_reference
def test_seam_installs_and_is_removed(ref):
    from optiland.rays.ray_aiming import iterative

    from optiland_amd import analysis_seams as seams

    was_enabled = bool(seams._ORIG)
    seams.disable()
    stock = iterative.IterativeRayAimer.aim_rays
    assert stock is not seams._iterative_aim_rays
    seams.enable()
    try:
        assert "aim" not in seams.SKIPPED
        assert {"aim", "aim_fallback"} <= set(seams.STATS)
        assert iterative.IterativeRayAimer.aim_rays is seams._iterative_aim_rays
        assert seams._ORIG["aim"] is stock
    finally:
        seams.disable()
    assert iterative.IterativeRayAimer.aim_rays is stock
    if was_enabled:
        seams.enable()


def _relay(be):
    from optiland import optic as optic_mod
    lens = optic_mod.Optic(name="FiniteRelay")
    lens.surfaces.add(index=0, radius=be.inf, thickness=60.0)
    lens.surfaces.add(index=1, radius=42.0, thickness=6.0, material="N-BK7")
    lens.surfaces.add(index=2, radius=-38.0, thickness=5.0)
    lens.surfaces.add(index=3, radius=be.inf, thickness=4.0, is_stop=True)
    lens.surfaces.add(index=4, radius=33.0, thickness=5.0, material="N-SF5")
    lens.surfaces.add(index=5, radius=-70.0, thickness=55.0)
    lens.surfaces.add(index=6)
    lens.set_aperture(aperture_type="objectNA", value=0.12)
    lens.fields.set_type(field_type="object_height")
    for y in (0.0, 7.0, 10.0):
        lens.fields.add(y=y)
    lens.wavelengths.add(value=0.55, is_primary=True)
    lens.ray_tracer.set_aiming("iterative", 20, 1e-8)
    return lens


@needs_reference
def test_seam_declines_on_the_cpu_and_under_hip_on_cpu(hip_on_cpu, tmp_path, monkeypatch):
    """torch on the CPU: with the drop-in forced on (`hip_on_cpu`) the engines of the CPU suite
    have no `ol_aim_rays`, without it the optic is not served -- either way the reference's own
    solve runs, `aim_fallback` moves and `aim` does not, and the trace is the fixture's."""
    from optiland_amd import analysis_seams as seams
    from optiland_amd import integration

    be = hip_on_cpu
    log = tmp_path / "seams.log"
    monkeypatch.setenv("OPTILAND_HIP_SEAM_LOG", str(log))
    c = RA.case("relay_h07")
    for force, why in ((True, "an engine without ol_aim_rays"), (False, "not served")):
        integration.enable(device="cpu", force=force)
        try:
            before = dict(seams.STATS)
            rays = _relay(be).trace(0.0, 0.7, 0.55, 3, "hexapolar")
            assert seams.STATS["aim_fallback"] == before["aim_fallback"] + 1
            assert seams.STATS["aim"] == before["aim"]
            assert why in log.read_text()
            got = np.stack([np.asarray(be.to_numpy(v), dtype=np.float64)
                            for v in (rays.x, rays.y, rays.z)])
            assert np.all(np.max(np.abs(got - c["image"][:3]), axis=0) <= RA.image_bound(c))
        finally:
            integration.disable()
        log.write_text("")


@needs_reference
def test_paraxial_start_scalars_whatever_the_aiming_mode(ref):
    """The scalars the seam hands the kernel for the paraxial start of an optic in ITERATIVE mode
    are the ones its table carries when packed under paraxial aiming (the fixture's table) -- and
    packing in iterative mode still leaves `table.raygen` empty."""
    from optiland.samples.objectives import WideAngle100FOV

    from optiland_amd import packer

    be = ref
    be.set_backend("numpy")
    lens = WideAngle100FOV()
    table = packer.pack_optic(lens, wavelengths=[float(lens.primary_wavelength)])
    assert not table.raygen and table.stop_index == RA.case("wa100_h07")["stop"]
    raygen, fields = packer.paraxial_start_scalars(lens, table)
    assert not table.raygen and not table.fields
    want = RA.table("wa100")
    assert set(raygen) == set(want.raygen)
    for k, v in want.raygen.items():
        assert raygen[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k
    assert [tuple(f) for f in fields] == [tuple(f) for f in want.fields]
