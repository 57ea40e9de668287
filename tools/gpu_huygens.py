#!/usr/bin/env python
"""Measure the Huygens-Fresnel summation (`ol_huygens_psf`) on the GPU -> profiles/huygens.txt.

    python tools/gpu_huygens.py [--sums-only]

* the kernel sum at num_rays 128 / image 128 (~12.9k pupil samples x 16384 pixels, ~2.1e8
  terms) and at 64 / 64, on the Cooke triplet's own pupil (fp64 wavefront, field (0, 1)):
  device-event time per call, terms per second;
* the same sum written the way the reference's `TorchSummation.compute` does it (batches of
  1024 pixels x all rays of complex128 temporaries, psf/huygens_fresnel_strategies.py:
  217-274, restated here from the formula), on the same GPU, and the largest difference;
* the stand-alone `HuygensPSF` end to end;
* (unless --sums-only) the fp64 VALU instructions per term of the partial-sum kernel's
  inner loop, from the gfx950 ISA (tools/asm_stats.py on a --save-temps compile).
Kernel times under rocprofv3: run `rocprofv3 --kernel-trace --stats -- python
tools/gpu_huygens.py --sums-only` separately.
"""

from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from optiland_amd import load_system  # noqa: E402
from optiland_amd import tracer as tr  # noqa: E402
from optiland_amd.engine import huygens_sum  # noqa: E402
from optiland_amd.wavefront import HuygensPSF  # noqa: E402

DEV = "cuda:0"
WL = 0.55


def torch_reference_sum(ix, iy, iz, px, py, pz, amp, opd, wavelength, Rp, batch=1024):
    k = 2.0 * torch.pi / wavelength
    px, py, pz, amp, opd = (v.reshape(1, -1) for v in (px, py, pz, amp, opd))
    fx, fy, fz = ix.flatten(), iy.flatten(), iz.flatten()
    field = torch.zeros(fx.numel(), dtype=torch.complex128, device=ix.device)
    for i in range(0, fx.numel(), batch):
        x, y, z = (v[i:i + batch].reshape(-1, 1) for v in (fx, fy, fz))
        dx, dy, dz = x - px, y - py, z - pz
        R = torch.sqrt(dx ** 2 + dy ** 2 + dz ** 2)
        wave = torch.exp(1j * k * R) / R
        cos_theta = (dx * (px / Rp) + dy * (py / Rp) + dz * (pz / Rp)) / R
        q = 0.5 * (1.0 + cos_theta)
        field[i:i + batch] = torch.sum(amp * torch.exp(-1j * k * opd) * wave * q, dim=1)
    return (torch.abs(field) ** 2).reshape(ix.shape)


def device_ms(fn, reps):
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


def inputs(tracer, num_rays, image_size):
    psf = HuygensPSF(tracer, (0.0, 1.0), WL, num_rays=num_rays, image_size=image_size)
    d = psf.wavefront.data
    image = psf._get_image_coordinates(d.opd.device)
    return (*image, d.pupil_x, d.pupil_y, d.pupil_z, torch.sqrt(d.intensity),
            d.opd * WL * 1e-3, WL * 1e-3, float(d.radius))


def golden_report():
    """Largest |kernel - reference| / peak over the golden compute() calls."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "huygens.npz")))
    worst = 0.0
    for case in g["cases"]:
        for k in range(int(g[f"{case}/n_calls"])):
            a = [torch.as_tensor(g[f"{case}/call{k}/{n}"], device=DEV) for n in
                 ("image_x", "image_y", "image_z", "pupil_x", "pupil_y", "pupil_z", "pupil_amp",
                  "pupil_opd")]
            want = g[f"{case}/call{k}/out"]
            got = huygens_sum(*a, float(g[f"{case}/call{k}/wavelength"]),
                              float(g[f"{case}/call{k}/Rp"])).cpu().numpy()
            worst = max(worst, float(np.max(np.abs(got - want)) / np.max(want)))
    print(f"golden compute() calls (the reference's fp64 torch sum): max |diff| / peak "
          f"{worst:.2e}")


def isa_report():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(ROOT, "optiland_amd", "csrc", "huygens.hip")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                               "-ffp-contract=on", "-fno-math-errno", "--save-temps", "-c", src,
                               "-o", os.path.join(tmp, "h.o")], cwd=tmp)
        asm = os.path.join(tmp, "huygens-hip-amdgcn-amd-amdhsa-gfx950.s")
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "asm_stats.py"),
                                       asm, "huygens_partial"], text=True)
    print(out.rstrip())
    m = re.search(r"loop depth 1: valu\s+(\d+).*?f64\s+(\d+)", out)
    if m:
        valu, f64 = int(m.group(1)), int(m.group(2))
        print(f"inner loop, 2 pixels per lane: {valu / 2:.1f} VALU instructions per term, "
              f"{f64 / 2:.1f} of them fp64")


def main():
    sums_only = "--sums-only" in sys.argv
    tracer = tr.HipRayTracer(load_system("cooke_generic"), DEV, dtype=torch.float64)
    print(f"device: {torch.cuda.get_device_name(0)}")
    for num_rays, image_size, reps in ((128, 128, 20), (64, 64, 50)):
        args = inputs(tracer, num_rays, image_size)
        n, m = args[3].numel(), args[0].numel()
        ms, best = device_ms(lambda: huygens_sum(*args), reps)
        print(f"num_rays {num_rays} / image {image_size}: {n} pupil samples x {m} pixels = "
              f"{n * m:.3e} terms; ol_huygens_psf {ms:.3f} ms median ({best:.3f} min) "
              f"= {n * m / ms / 1e9:.3f} Tterm/s")
        if sums_only:
            continue
        ref = torch_reference_sum(*args)
        got = huygens_sum(*args)
        diff = float((got - ref).abs().max() / ref.max())
        rms, rbest = device_ms(lambda: torch_reference_sum(*args), 3 if num_rays == 128 else 10)
        print(f"    reference-style torch sum (batches of 1024 pixels): {rms:.2f} ms median "
              f"({rbest:.2f} min), {rms / ms:.0f}x the kernel; max |diff| / peak {diff:.2e}")
    if not sums_only:
        for num_rays, image_size in ((128, 128), (64, 64)):
            HuygensPSF(tracer, (0.0, 1.0), WL, num_rays=num_rays, image_size=image_size)
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                p = HuygensPSF(tracer, (0.0, 1.0), WL, num_rays=num_rays, image_size=image_size)
                float(p.psf[0, 0])
                ts.append((time.perf_counter() - t0) * 1e3)
            print(f"HuygensPSF(cooke, (0, 1), num_rays={num_rays}, image_size={image_size}) end "
                  f"to end: {np.median(ts):.2f} ms median ({min(ts):.2f} min), strehl "
                  f"{p.strehl_ratio():.6f}")
        golden_report()
        isa_report()


if __name__ == "__main__":
    main()
