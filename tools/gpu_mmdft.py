#!/usr/bin/env python
"""Measure the MMDFT PSF (`ol_mmdft_psf`) on the GPU -> profiles/mmdft.txt.

    python tools/gpu_mmdft.py [--calls-only]

* the whole call (`engine.mmdft_psf`, device-event time, median and minimum) at (N 45, M 128),
  (N 64, M 512), (N 90, M 512), (N 128, M 1024), (N 181, M 2048) and for a batch of 25 pupils at (N 45, M 128), on seeded random
  pupils, with the fp64 FMA rate of the two products (8 real FMAs per complex term pair:
  8 (N^2 M + N M^2) flop);
* the same PSF the way the reference's torch backend gets it (psf/mmdft.py:157-283, restated
  from the formula: `outer`, `exp`, two complex128 `matmul`s, |.|^2 * 100 / norm) on the same
  GPU and inputs, and the largest difference between the two;
* (unless --calls-only) the errors against the exact and the recorded fixtures.
Kernel times: run `rocprofv3 --kernel-trace --stats -- python tools/gpu_mmdft.py --calls-only`
separately (a run of its own: tracing slows the host).
"""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from optiland_amd.engine import mmdft_psf  # noqa: E402
from tests import _mmdft as MM  # noqa: E402

DEV = "cuda:0"
# (N, M, pupils, repetitions)
SHAPES = ((45, 128, 1, 200), (64, 512, 1, 200), (90, 512, 1, 200), (128, 1024, 1, 100),
          (181, 2048, 1, 50), (45, 128, 25, 200))


def torch_reference_psf(pupil, pad, m):
    """psf/mmdft.py:173-177 and :266-282 with torch on the device, per pupil."""
    n = pupil.shape[-1]
    # (fp64 coordinates: the products are complex128 from the start, as on the reference's
    # float64 backend)
    cp = torch.arange(n, device=pupil.device, dtype=torch.float64) - n // 2
    ci = torch.arange(m, device=pupil.device, dtype=torch.float64) - m // 2
    right = torch.exp(-2j * torch.pi * torch.outer(cp, ci) / pad).to(torch.complex128)
    left = torch.exp(-2j * torch.pi * torch.outer(ci, cp) / pad).to(torch.complex128)
    image = torch.matmul(left, torch.matmul(pupil, right))
    psf = image * torch.conj(image)
    return torch.real(psf) * 100 / torch.sum(torch.abs(pupil) > 0) ** 2


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


def fixture_report():
    g = MM.exact()
    for case in MM.cases(g):
        pupil, pad, m = g[f"{case}/pupil"], float(g[f"{case}/pad_size"]), int(g[f"{case}/image_size"])
        psf, field = mmdft_psf(torch.as_tensor(pupil, device=DEV), pad, m, want_field=True)
        b = MM.field_bound(pupil.shape[0], float(g[f"{case}/sum_abs"]))
        err = float(np.abs(field.cpu().numpy() - g[f"{case}/field"]).max())
        perr = float(np.abs(psf.cpu().numpy() - g[f"{case}/psf"]).max() / g[f"{case}/psf"].max())
        print(f"exact {case:10s}: max |G - G_exact| {err:.3e} = {err / b:.4f} B (NumPy formula "
              f"{float(g[case + '/numpy_field_err']) / b:.4f} B); psf {perr:.2e} of the peak")
    g = MM.golden()
    for case in MM.cases(g):
        want = g[f"{case}/psf"]
        got = mmdft_psf(torch.as_tensor(g[f"{case}/pupil"], device=DEV),
                        float(g[f"{case}/pad_size"]), want.shape[0]).cpu().numpy()
        print(f"reference {case:18s}: max |psf - recorded| / peak "
              f"{float(np.abs(got - want).max() / want.max()):.2e}")


def main():
    calls_only = "--calls-only" in sys.argv
    print(f"device: {torch.cuda.get_device_name(0)}")
    for n, m, batch, reps in SHAPES:
        pupils = torch.as_tensor(MM.random_pupil(n, seed=n + m, batch=batch), device=DEV)
        pads = [m + 0.65 + k for k in range(batch)]
        flop = 8.0 * batch * (n * n * m + n * m * m)
        ms, best = device_ms(lambda: mmdft_psf(pupils, pads, m), reps)
        print(f"N {n} M {m} x {batch}: mmdft_psf {ms:.4f} ms median ({best:.4f} min) per call, "
              f"{flop / ms / 1e9:.2f} TFLOP/s fp64 over the whole call")
        if calls_only:
            continue

        def route():
            return [torch_reference_psf(pupils[k], pads[k], m) for k in range(batch)]

        rms, rbest = device_ms(route, max(5, reps // 4))
        ref = torch.stack(route())
        diff = float((mmdft_psf(pupils, pads, m) - ref).abs().max() / ref.max())
        print(f"    reference-style torch route: {rms:.4f} ms median ({rbest:.4f} min), "
              f"{rms / ms:.2f} x the call; max |diff| / peak {diff:.2e}")
    if not calls_only:
        fixture_report()


if __name__ == "__main__":
    main()
