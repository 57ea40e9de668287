"""Iterative ray aiming on the MI355X (`ol_aim_rays`, csrc/ray_aim.hip) against the reference's
recorded solves (tests/golden/ray_aim.npz, tools/make_golden_ray_aim.py): the contract of a solve
by an independent re-trace, launch planes and image-plane hits against the fixture within the
bounds of tests/_ray_aim.py, step counts, both ways to start, the two status words, ragged
shapes, and the unmodified reference API with the drop-in enabled.

Measured on the MI355X (profiles/ray_aim.txt): launch planes within 1.3e-14 and image-plane hits
within 2.9e-14 of the fixture over all twelve cases (bounds: 3.4e-10 ... 1.3e-6), every re-traced
ray within 0.98 tol of its target, step counts equal to the reference's in every case."""

import numpy as np
import pytest
import torch

from optiland_amd import _capi
from tests import _live
from tests import _ray_aim as RA

pytestmark = pytest.mark.gpu

CASES = RA.cases()
PARAXIAL_OK = [c for c in CASES if c.startswith(("wa100", "relay")) or c.endswith("h00")]
DEV = "cuda"


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from optiland_amd.engine import HipSystem
    made = {}

    def get(system):
        if system not in made:
            made[system] = HipSystem(RA.table(system), DEV)
        return made[system]
    yield get
    for e in made.values():
        e.close()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _host(planes):
    return np.stack([p.cpu().numpy() for p in planes])


def _solve(eng, c, *, pupil=None, guess="fixture", **over):
    pupil = c["pupil"] if pupil is None else pupil
    kw = dict(first=c["first"], stop=c["stop"], stop_radius=c["r_stop"], jacobian=c["jacobian"],
              infinite=c["infinite"], tol=c["tol"], max_iter=c["max_iter"])
    if isinstance(guess, str):
        kw["guess"] = [_dev(p) for p in c["guess"]]
    elif guess is None:
        kw["field"] = (0.0, c["hy"])
    else:
        kw["guess"] = [_dev(p) for p in guess]
    kw.update(over)
    return eng.aim_rays(_dev(pupil[0]), _dev(pupil[1]), 0, **kw)


def _trace(eng, launch, first, last):
    """The final global state of `ol_trace` over [first, last] from the launch planes (6, n)."""
    n = launch.shape[1]
    rays = [_dev(p) for p in launch] + [torch.ones(n, dtype=torch.float64, device=DEV),
                                        torch.zeros(n, dtype=torch.float64, device=DEV)]
    eng.trace(rays, 0, record=False, first=first, last=last, write_rays=True)
    return _host(rays)


@pytest.mark.parametrize("name", CASES)
def test_contract_reference_and_step_counts(name, engines):
    c = RA.case(name)
    eng = engines(c["system"])
    out, updates = _solve(eng, c, want_updates=True)
    assert int(eng._status.item()) == 0
    solved, updates = _host(out), updates.cpu().numpy()
    # (1) the contract: every ray, re-traced to the stop by ol_trace and brought into the stop's
    # frame, lands within tol of (Px, Py) r_stop -- 8 ulp of slack for the frame round trip
    g = _trace(eng, solved, c["first"], c["stop"])
    lx, ly, _lz = RA.stop_local(c["table"], c["stop"], g[0], g[1], g[2])
    miss = np.hypot(lx - c["pupil"][0] * c["r_stop"], ly - c["pupil"][1] * c["r_stop"])
    slack = RA.contract_slack(c, lx, ly)
    # (2) against the reference: launch planes, and the image-plane hits of the following trace
    d_launch = np.max(np.abs(solved - c["solved"]), axis=0)
    image = _trace(eng, solved, 0, c["table"].num_surfaces - 1)
    d_image = np.max(np.abs(image[:3] - c["image"][:3]), axis=0)
    print(f"{name}: miss max {miss.max():.3e} (tol {c['tol']:g}), launch {d_launch.max():.3e} "
          f"(bound {RA.launch_bound(c).min():.3e}), image {d_image.max():.3e} "
          f"(bound {RA.image_bound(c).min():.3e}), steps max {updates.max()} "
          f"(reference passes {c['passes']})")
    assert np.all(miss <= c["tol"] + slack), (miss.max(), c["tol"])
    assert np.all(d_launch <= RA.launch_bound(c)), d_launch.max()
    assert np.all(d_image <= RA.image_bound(c)), d_image.max()
    # (3) the same arithmetic in the same order: as many passes as the reference made
    assert updates.max() == c["passes"]


@pytest.mark.parametrize("name", PARAXIAL_OK)
def test_paraxial_start_generated_or_given(name, engines):
    c = RA.case(name)
    eng = engines(c["system"])
    given = _host(_solve(eng, c, guess=c["paraxial"]))
    made = _host(_solve(eng, c, guess=None))
    bound = RA.launch_bound(c)
    assert np.all(np.max(np.abs(made - given), axis=0) <= bound)
    assert np.all(np.max(np.abs(made - c["solved"]), axis=0) <= bound)


def test_status_words_are_the_references_errors(engines):
    c = RA.case("wa100_h10")
    eng = engines("wa100")
    with pytest.raises(ValueError) as err:
        _solve(eng, c, max_iter=1)
    assert str(err.value) == "Iterative aimer failed to converge."
    guess = c["guess"].copy()
    guess[1, 5] = np.nan
    with pytest.raises(ValueError) as err:
        _solve(eng, c, guess=guess)
    assert str(err.value) == ("Initial ray aiming guess produced NaNs. "
                              "Consider using the 'robust' method instead.")
    # the bits themselves, and the other rays of that call
    out = _solve(eng, c, guess=guess, check_status=False)
    assert int(eng._status.item()) == _capi.AIM_NAN_GUESS | _capi.AIM_NOT_CONVERGED
    keep = np.arange(guess.shape[1]) != 5
    assert np.all(np.max(np.abs(_host(out) - c["solved"]), axis=0)[keep] <= RA.launch_bound(c)[keep])
    # a robust lens from the paraxial state: a NaN in the first error -- what its recursion lives on
    c170 = RA.case("wa170_h10")
    with pytest.raises(ValueError, match="produced NaNs"):
        _solve(engines("wa170"), c170, guess=None)
    # ordinary status words: the engine goes on
    assert np.all(np.max(np.abs(_host(_solve(eng, c)) - c["solved"]), axis=0) <= RA.launch_bound(c))


def test_shapes_one_ray_one_past_a_wave_and_none(engines):
    """n = 1, n = 65 (one lane past a wave: two workgroups, the second with one ray) and n = 0.
    A ray's solution does not depend on the rays it shares a wave with."""
    c = RA.case("relay_h10")
    eng = engines("relay")
    want = _host(_solve(eng, c))
    idx = np.arange(65) % c["pupil"].shape[1]
    out, updates = _solve(eng, c, pupil=c["pupil"][:, idx], guess=c["guess"][:, idx],
                          want_updates=True)
    assert np.array_equal(_host(out), want[:, idx])
    assert np.array_equal(updates.cpu().numpy(), c["updates"][idx])
    one = _host(_solve(eng, c, pupil=c["pupil"][:, 36:], guess=c["guess"][:, 36:]))
    assert one.shape == (6, 1) and np.array_equal(one[:, 0], want[:, 36])
    none, updates = _solve(eng, c, pupil=c["pupil"][:, :0], guess=c["guess"][:, :0],
                           want_updates=True)
    assert all(p.numel() == 0 for p in none) and updates.numel() == 0
    # the generating start, ragged as well
    made = _host(_solve(eng, c, pupil=c["pupil"][:, idx], guess=None))
    assert np.all(np.max(np.abs(made - want[:, idx]), axis=0) <= RA.launch_bound(c)[idx])


def test_standalone_tracer_entry(engines):
    from optiland_amd import tracer as tr
    c = RA.case("wa100_h07")
    t = tr.HipRayTracer(c["table"], DEV, dtype=torch.float64, engine=engines("wa100"))
    out = t.aim_rays(0.0, c["hy"], c["pupil"][0], c["pupil"][1], c["wavelength"],
                     stop_radius=c["r_stop"], jacobian=c["jacobian"], tol=c["tol"],
                     max_iter=c["max_iter"])
    assert np.all(np.max(np.abs(_host(out) - c["solved"]), axis=0) <= RA.launch_bound(c))
    with pytest.raises(ValueError, match="failed to converge"):
        t.aim_rays(0.0, 1.0, c["pupil"][0], c["pupil"][1], c["wavelength"],
                   stop_radius=c["r_stop"], jacobian=c["jacobian"], max_iter=1)


# ------------------------------------------------------------------ the unmodified reference API
@pytest.fixture
def on_device():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if _live.reference_root() is None:
        pytest.skip("reference package not staged (oracle/stage_reference.py)")
    from optiland_amd import analysis_seams as seams
    from optiland_amd import integration
    be = _live.import_reference()
    be.set_backend("torch")
    be.set_device("cuda")
    be.set_precision("float64")
    integration.enable()
    try:
        yield be, seams.STATS
    finally:
        integration.disable()
        be.set_precision("float64")
        be.set_device("cpu")
        be.set_backend("numpy")


@pytest.mark.parametrize("sample,name", [("WideAngle100FOV", "wa100_h07"),
                                         ("ProjectionLens120FOV", "proj120_h07")])
def test_through_the_reference_api(sample, name, on_device):
    from optiland.samples import objectives

    be, stats = on_device
    c = RA.case(name)
    before = dict(stats)
    lens = getattr(objectives, sample)()
    rays = lens.trace(0.0, c["hy"], c["wavelength"], 3, "hexapolar")
    assert stats["aim"] >= before["aim"] + 1
    assert stats["aim_fallback"] == before["aim_fallback"]
    comp = lens.ray_tracer.__dict__.get("_hip_companion")
    assert comp is not None and comp.last_path == "reference-rays"
    got = np.stack([np.asarray(be.to_numpy(v), dtype=np.float64) for v in (rays.x, rays.y, rays.z)])
    d = np.max(np.abs(got - c["image"][:3]), axis=0)
    print(f"{sample}: {stats['aim'] - before['aim']} solves on the device (the reference made "
          f"{c['solves']}), image {d.max():.3e} (bound {RA.image_bound(c).min():.3e})")
    assert np.all(d <= RA.image_bound(c)), d.max()
