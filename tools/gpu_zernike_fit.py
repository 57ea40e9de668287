#!/usr/bin/env python
"""Measure the Zernike fit and the sampled MTF (`ol_zernike_fit`, `ol_sampled_mtf`) on the GPU
-> profiles/zernike_fit.txt.

    python tools/gpu_zernike_fit.py [--kernels-only]

* `engine.zernike_fit` at 721 x 37 (hexapolar, 15 rings) and 12 868 x 37 (uniform grid of
  `num_rays` 128), `engine.sampled_mtf` at 740 points x 33 frequencies and 12 868 x 64: device-event
  time per call (all launches and the workspace), on the Cooke triplet's own OPD map;
* the stand-alone `ZernikeOPD(tracer)` and `SampledMTF(tracer)` + `calculate_mtf` (wall clock);
* (unless --kernels-only, and when the reference package is staged) on the same box: the
  reference's `SampledMTF.calculate_mtf`, `ZernikeOPD` and `MTFVsField` on its NumPy backend, and
  on its fp64 torch backend on the device through the drop-in -- with the two seams of this
  feature OFF (every other seam on: what the commit before this feature does) and ON -- with the
  largest difference between the drop-in's numbers and the NumPy backend's.
Kernel times under rocprofv3: run `rocprofv3 --kernel-trace --stats -- python
tools/gpu_zernike_fit.py --kernels-only` separately.
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
from optiland_amd.engine import sampled_mtf, zernike_fit  # noqa: E402
from optiland_amd.mtf import SampledMTF, pupil_shifts  # noqa: E402
from optiland_amd.wavefront import Wavefront, ZernikeOPD  # noqa: E402

DEV = "cuda:0"
FIELD = (0.0, 0.7)


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


def wall_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), out


def standalone(tracer):
    w = float(tracer.table.wavelengths[tracer.table.reference_wavelength_index()])
    for dist, num, freqs in (("hexapolar", 15, None), ("uniform", 32, 33), ("uniform", 128, 64)):
        wf = Wavefront(tracer, FIELD, w, num_rays=num, distribution=dist)
        x, y = tracer._dev(wf.distribution.x), tracer._dev(wf.distribution.y)
        opd, inten = wf.data.opd, wf.data.intensity
        n = x.numel()
        if freqs is None or num == 128:
            ms, best = device_ms(lambda: zernike_fit(x, y, opd, "fringe", 37, device=DEV), 200)
            print(f"engine.zernike_fit {n} points x 37 terms: {ms:.3f} ms median ({best:.3f} min, "
                  f"device events, no read-back)")
        if freqs is not None:
            c, _ = zernike_fit(x, y, opd, "fringe", 37, device=DEV)
            m = SampledMTF(tracer, FIELD, w, num_rays=num)
            sh = torch.as_tensor(pupil_shifts([(0.0, f) for f in np.linspace(0.0, 80.0, freqs)],
                                              w, m.xpd, m.xpl), device=DEV)
            ms, best = device_ms(lambda: sampled_mtf(c, "fringe", x, y, opd, inten, sh,
                                                     device=DEV), 200)
            print(f"engine.sampled_mtf {n} points x {freqs} frequencies: {ms:.3f} ms median "
                  f"({best:.3f} min, device events)")
    ms, best, _ = wall_ms(lambda: float(ZernikeOPD(tracer, FIELD, w).coeffs[3]), 50)
    print(f"ZernikeOPD(tracer) 721 points x 37 terms end to end: {ms:.3f} ms median ({best:.3f} min, "
          f"wall clock)")
    fr = [(0.0, float(f)) for f in np.linspace(0.0, 80.0, 33)]
    ms, best, _ = wall_ms(lambda: float(SampledMTF(tracer, FIELD, w, num_rays=32)
                                        .calculate_mtf(fr)[5]), 50)
    print(f"SampledMTF(tracer, num_rays=32) + calculate_mtf(33 frequencies) end to end: {ms:.3f} ms "
          f"median ({best:.3f} min, wall clock)")


def reference_side():
    try:
        from tests import _live
        be = _live.import_reference()
    except ImportError as exc:
        print(f"reference package not staged ({exc}): reference timings not measured")
        return
    from optiland.analysis import MTFVsField
    from optiland.mtf import SampledMTF as RefMTF
    from optiland.samples.objectives import CookeTriplet
    from optiland.wavefront import ZernikeOPD as RefZernikeOPD

    from optiland_amd import analysis_seams as seams
    from optiland_amd import integration

    fr = [(0.0, float(f)) for f in np.linspace(0.0, 80.0, 33)]

    def arr(v):
        return np.array([float(be.to_numpy(t)) for t in v])

    def run(tag, reps):
        lens = CookeTriplet()
        w = lens.primary_wavelength
        m = RefMTF(lens, FIELD, w, num_rays=32)
        ms, best, mtf = wall_ms(lambda: m.calculate_mtf(fr), reps, warm=1)
        print(f"{tag}: SampledMTF(num_rays=32).calculate_mtf(33 frequencies) {ms:.3f} ms median "
              f"({best:.3f} min), {ms / 33:.3f} ms per frequency")
        ms, best, z = wall_ms(lambda: RefZernikeOPD(lens, FIELD, w), reps, warm=1)
        print(f"{tag}: ZernikeOPD(15 rings, 37 terms) {ms:.3f} ms median ({best:.3f} min)")
        ms, best, v = wall_ms(lambda: MTFVsField(lens, frequencies=[10.0, 30.0], num_fields=4,
                                                 num_rays=32), max(reps // 4, 1), warm=1)
        print(f"{tag}: MTFVsField(2 frequencies, 4 fields, num_rays=32) {ms:.1f} ms median "
              f"({best:.1f} min)")
        return arr(mtf), np.asarray(be.to_numpy(z.coeffs), dtype=np.float64)

    be.set_backend("numpy")
    want_mtf, want_c = run("reference, NumPy backend (CPU of this box)", 3)
    be.set_backend("torch")
    be.set_device("cuda")
    be.set_precision("float64")
    integration.enable()
    try:
        held = {k: seams._ORIG.get(k) for k in ("zfit", "smtf")}
        import importlib
        for k, fn in held.items():        # the two seams of this feature off, the others on
            mod, cls, meth = seams._SEAMS[k][:3]
            setattr(getattr(importlib.import_module(mod), cls), meth, fn)
        run("drop-in, the Zernike-fit and sampled-MTF seams OFF (as before this feature)", 3)
        for k in held:
            mod, cls, meth = seams._SEAMS[k][:3]
            setattr(getattr(importlib.import_module(mod), cls), meth,
                    getattr(seams, seams._SEAMS[k][4]))
        before = dict(seams.STATS)
        got_mtf, got_c = run("drop-in, every seam on", 20)
        print("seam calls: " + ", ".join(f"{k} {seams.STATS[k] - before[k]}" for k in
                                         ("zfit", "zfit_fallback", "smtf", "smtf_fallback")))
        print(f"max |drop-in - NumPy backend|: sampled MTF {np.abs(got_mtf - want_mtf).max():.3e}, "
              f"Zernike coefficients {np.abs(got_c - want_c).max():.3e}")
    finally:
        integration.disable()
        be.set_backend("numpy")


def main():
    print(f"device: {torch.cuda.get_device_name(0)}")
    tracer = tr.HipRayTracer(load_system("cooke_generic"), DEV, dtype=torch.float64)
    standalone(tracer)
    if "--kernels-only" not in sys.argv:
        reference_side()


if __name__ == "__main__":
    main()
