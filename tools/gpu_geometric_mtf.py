#!/usr/bin/env python
"""Measure the geometric MTF (`ol_geometric_mtf`) on the GPU -> profiles/geometric_mtf.txt.

    python tools/gpu_geometric_mtf.py [--kernels-only]

* `engine.geometric_mtf` on the Cooke triplet's own hits, default case (3 fields, num_rays 100
  uniform = 7668 hits per field, 256 frequencies) and a large one (num_rays 1000, ~7.9e5 hits
  per field): device-event time per call (three kernels + the workspace);
* the stand-alone `GeometricMTF(tracer)` end to end (wall clock, ends in a read-back);
* (unless --kernels-only, and when the reference package is staged) on the same box: the
  reference's `GeometricMTF` on its NumPy backend, on its torch backend on the device (time, or
  the exception it raises), and through the drop-in (`integration.enable()`), with the largest
  difference between the drop-in's curves and the NumPy backend's.
Kernel times under rocprofv3: run `rocprofv3 --kernel-trace --stats -- python
tools/gpu_geometric_mtf.py --kernels-only` separately.
"""

from __future__ import annotations

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from optiland_amd import load_system  # noqa: E402
from optiland_amd import tracer as tr  # noqa: E402
from optiland_amd.engine import geometric_mtf  # noqa: E402
from optiland_amd.mtf import GeometricMTF  # noqa: E402

DEV = "cuda:0"
CASES = (("default", 100, 200), ("large", 1000, 50))


def device_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return float(np.median(times)), float(np.min(times))


def wall_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times))


def standalone(tracer):
    for name, num_rays, reps in CASES:
        m = GeometricMTF(tracer, num_rays=num_rays)
        curves = [c for x, y in m.data for c in (y, x)]
        freq = torch.as_tensor(m.freq, device=DEV)
        scale = torch.as_tensor(m.diff_limited_mtf, device=DEV)
        ms, best = device_ms(lambda: geometric_mtf(curves, freq, scale), reps)
        print(f"{name}: {len(curves)} curves x {curves[0].numel()} hits, {freq.numel()} "
              f"frequencies: engine.geometric_mtf {ms:.3f} ms median ({best:.3f} min, device "
              f"events, flag read-back included)")
        ms, best = wall_ms(lambda: float(GeometricMTF(tracer, num_rays=num_rays).mtf[0][0][1]),
                           reps)
        print(f"{name}: GeometricMTF(tracer, num_rays={num_rays}) end to end {ms:.3f} ms median "
              f"({best:.3f} min, wall clock)")


def reference_side():
    sys.path.insert(0, ROOT)
    try:
        from tests import _live
        be = _live.import_reference()
    except ImportError as exc:
        print(f"reference package not staged ({exc}): reference timings not measured")
        return
    from optiland.mtf import GeometricMTF as RefMTF
    from optiland.samples.objectives import CookeTriplet

    from optiland_amd import analysis_seams as seams
    from optiland_amd import integration

    def timed(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), out

    be.set_backend("numpy")
    lens = CookeTriplet()
    ms, best, ref = timed(lambda: RefMTF(lens), 3)
    print(f"reference, NumPy backend (CPU of this box): GeometricMTF(CookeTriplet()) {ms:.1f} ms "
          f"median ({best:.1f} min)")
    want = np.array([[np.asarray(t), np.asarray(s)] for t, s in ref.mtf])
    be.set_backend("torch")
    be.set_device("cuda")
    be.set_precision("float64")
    lens = CookeTriplet()
    try:
        ms, best, _ = timed(lambda: RefMTF(lens), 3)
        print(f"reference, torch backend on the device, no drop-in: {ms:.1f} ms median "
              f"({best:.1f} min)")
    except Exception as exc:  # noqa: BLE001 - the text is the finding
        print(f"reference, torch backend on the device, no drop-in: raises "
              f"{type(exc).__name__}: {str(exc).splitlines()[0][:300]}")
    integration.enable()
    try:
        lens = CookeTriplet()
        before = dict(seams.STATS)
        ms, best, got = timed(lambda: RefMTF(lens), 50)
        n = seams.STATS["geo_mtf"] - before["geo_mtf"]
        fb = seams.STATS["geo_mtf_fallback"] - before["geo_mtf_fallback"]
        have = np.array([[t.cpu().numpy(), s.cpu().numpy()] for t, s in got.mtf])
        print(f"reference through the drop-in (fp64 torch backend on the device): {ms:.3f} ms "
              f"median ({best:.3f} min); seam calls {n}, fall-backs {fb}; max |drop-in - NumPy "
              f"backend| = {np.max(np.abs(have - want)):.3e}")
        for name, num_rays, reps in CASES[1:]:
            ms, best, _ = timed(lambda: RefMTF(lens, num_rays=num_rays), reps)
            print(f"reference through the drop-in, num_rays={num_rays}: {ms:.3f} ms median "
                  f"({best:.3f} min)")
    finally:
        integration.disable()
        be.set_backend("numpy")


def main():
    kernels_only = "--kernels-only" in sys.argv
    print(f"device: {torch.cuda.get_device_name(0)}")
    tracer = tr.HipRayTracer(load_system("cooke_generic"), DEV, dtype=torch.float64)
    standalone(tracer)
    if not kernels_only:
        reference_side()


if __name__ == "__main__":
    main()
