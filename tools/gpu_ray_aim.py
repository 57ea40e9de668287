#!/usr/bin/env python
"""Measure iterative ray aiming on the GPU (`ol_aim_rays`) -> profiles/ray_aim.txt.

    python tools/gpu_ray_aim.py [--quick] [--out FILE]

* the errors of every fixture case (tests/golden/ray_aim.npz): the worst miss of a re-traced ray
  on the stop plane against `tol`, launch planes and image-plane hits against the reference with
  their bounds (tests/_ray_aim.py), step counts;
* the `ol_aim_rays` call alone (host clock around a call that ends in the status read-back,
  median) at 37 rays and at 37 x 1024 rays;
* the time of one `Optic.trace(0, Hy, primary, 3, "hexapolar")` of the reference's four sample
  lenses with iterative / robust aiming, through the unmodified reference API on the torch
  backend (cuda, fp64) with the drop-in enabled -- NEW: as it is; OLD: the same process with
  `IterativeRayAimer.aim_rays` put back to the reference's own method, i.e. what the drop-in did
  before this seam existed (the reference's loop on device tensors; everything else -- the
  surface-group seam behind it, the cache wrapper's hashing -- is the same code in both arms).
  The sample lenses wrap their aimer in the reference's result cache: it is cleared before every
  timed call, so that each call solves.  Arms alternate; medians after one warm-up call each.
  (--quick: fewer repetitions, no Hy = 1 for the 170-degree lens in the old arm.)
"""

from __future__ import annotations

import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _live  # noqa: E402
from tests import _ray_aim as RA  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "ray_aim.txt")
LENSES = ("WideAngle100FOV", "ProjectionLens120FOV", "ProjectionLens160FOV", "WideAngle170FOV")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _host(planes):
    return np.stack([p.cpu().numpy() for p in planes])


def _kw(c):
    return dict(first=c["first"], stop=c["stop"], stop_radius=c["r_stop"], jacobian=c["jacobian"],
                infinite=c["infinite"], tol=c["tol"], max_iter=c["max_iter"])


def _trace(eng, launch, first, last):
    n = launch.shape[1]
    rays = [_dev(p) for p in launch] + [torch.ones(n, dtype=torch.float64, device=DEV),
                                        torch.zeros(n, dtype=torch.float64, device=DEV)]
    eng.trace(rays, 0, record=False, first=first, last=last, write_rays=True)
    return _host(rays)


def errors(say):
    from optiland_amd.engine import HipSystem

    say("## errors against tests/golden/ray_aim.npz (37 rays per case)")
    say("case          miss/tol   launch     (bound)    image      (bound)    steps (reference)")
    engines = {}
    for name in RA.cases():
        c = RA.case(name)
        eng = engines.setdefault(c["system"], HipSystem(c["table"], DEV))
        out, upd = eng.aim_rays(_dev(c["pupil"][0]), _dev(c["pupil"][1]), 0,
                                guess=[_dev(p) for p in c["guess"]], want_updates=True, **_kw(c))
        solved = _host(out)
        g = _trace(eng, solved, c["first"], c["stop"])
        lx, ly, _ = RA.stop_local(c["table"], c["stop"], g[0], g[1], g[2])
        miss = np.hypot(lx - c["pupil"][0] * c["r_stop"], ly - c["pupil"][1] * c["r_stop"])
        image = _trace(eng, solved, 0, c["table"].num_surfaces - 1)
        say(f"{name:12s}  {miss.max() / c['tol']:.3e}  "
            f"{np.max(np.abs(solved - c['solved'])):.3e}  ({RA.launch_bound(c).min():.3e})  "
            f"{np.max(np.abs(image[:3] - c['image'][:3])):.3e}  ({RA.image_bound(c).min():.3e})  "
            f"{int(upd.max())} ({c['passes']})")
    return engines


def call_times(say, engines, reps):
    say("")
    say("## the ol_aim_rays call (host clock to the status read-back, median of "
        f"{reps}; ms)")
    for name in ("wa100_h07", "wa170_h10", "relay_h10"):
        c = RA.case(name)
        eng = engines[c["system"]]
        for copies in (1, 1024):
            px, py = (_dev(np.tile(p, copies)) for p in c["pupil"])
            guess = [_dev(np.tile(p, copies)) for p in c["guess"]]
            times = []
            for k in range(reps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.aim_rays(px, py, 0, guess=guess, **_kw(c))
                times.append((time.perf_counter() - t0) * 1e3)
            say(f"{name:12s} n = {px.numel():6d}: {statistics.median(times[3:]):.3f} "
                f"(best {min(times[3:]):.3f})")


def trace_times(say, quick):
    be = _live.import_reference()
    from optiland.rays.ray_aiming.iterative import IterativeRayAimer
    from optiland.samples import objectives

    from optiland_amd import analysis_seams as seams
    from optiland_amd import integration

    be.set_backend("torch")
    be.set_device("cuda")
    be.set_precision("float64")
    integration.enable()
    new_method, old_method = IterativeRayAimer.aim_rays, seams._ORIG["aim"]
    assert new_method is seams._iterative_aim_rays
    say("")
    say("## Optic.trace(0, Hy, primary, 3, 'hexapolar') through the reference API, torch / cuda / "
        "fp64, drop-in enabled (ms per call, median; the aimer's result cache cleared per call)")
    say("lens                   Hy    new     old      old/new  solves  max |new - old| image")
    try:
        for label in LENSES:
            for hy in (0.7, 1.0):
                lens = getattr(objectives, label)()
                w = float(lens.primary_wavelength)
                slow = label == "WideAngle170FOV" and hy == 1.0
                if slow and quick:
                    reps_new, reps_old = 3, 0
                else:
                    reps_new, reps_old = (3, 1) if slow else ((3, 2) if quick else (7, 5))
                times = {"new": [], "old": []}
                hits, solves = {}, 0

                def one(arm):
                    nonlocal solves
                    IterativeRayAimer.aim_rays = new_method if arm == "new" else old_method
                    aimer = lens.ray_tracer.ray_generator.aimer
                    if hasattr(aimer, "clear_cache"):
                        aimer.clear_cache()
                    before = seams.STATS["aim"]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rays = lens.trace(0.0, hy, w, 3, "hexapolar")
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    if arm == "new":
                        solves = seams.STATS["aim"] - before
                    else:
                        assert seams.STATS["aim"] == before
                    hits[arm] = np.stack([np.asarray(be.to_numpy(v)) for v in
                                          (rays.x, rays.y, rays.z)])
                    return dt

                one("new")                       # warm-up (packs the table, loads the kernels)
                if reps_old:
                    one("old")
                for k in range(max(reps_new, reps_old)):
                    if k < reps_new:
                        times["new"].append(one("new"))
                    if k < reps_old:
                        times["old"].append(one("old"))
                new = statistics.median(times["new"])
                if reps_old:
                    old = statistics.median(times["old"])
                    diff = float(np.nanmax(np.abs(hits["new"] - hits["old"])))
                    say(f"{label:22s} {hy:.1f}  {new:7.2f} {old:9.2f} {old / new:7.1f}  "
                        f"{solves:5d}   {diff:.3e}")
                else:
                    say(f"{label:22s} {hy:.1f}  {new:7.2f}  (old arm not run)    {solves:5d}")
    finally:
        IterativeRayAimer.aim_rays = new_method
        integration.disable()
        be.set_device("cpu")
        be.set_backend("numpy")


def main():
    quick = "--quick" in sys.argv
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/gpu_ray_aim.py{' --quick' if quick else ''} on {torch.cuda.get_device_name(0)}")
    engines = errors(say)
    call_times(say, engines, 20 if quick else 100)
    for e in engines.values():
        e.close()
    if _live.reference_root() is None:
        say("(reference package not staged: no Optic.trace timings)")
    else:
        trace_times(say, quick)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
