#!/usr/bin/env python
"""Measure the Forbes one-surface launch on the GPU (`ol_trace_forbes`) -> profiles/forbes.txt.

    python tools/gpu_forbes.py [--quick] [--out FILE]

* the errors of every fixture case (tests/golden/forbes.npz) against their bounds
  (tests/_forbes.py), fp64 and fp32;
* the time of one `ol_trace_forbes` launch at N = 1e3, 1e5 and 1e7 rays, fp32 and fp64, on the Q
  surface (5 terms) and on the Q2D surface (the fixture's terms), both recording a row and writing
  the state back: 8 planes read, 16 written;
* beside each, the existing one-surface launch `ol_trace(first = last = s)` on the even-asphere
  surface of aspheric_singlet at the same N and dtype with the same traffic -- a kernel this file's
  subject did not touch;
* bytes moved per second (24 planes x N x element size over the time).
Times: device events around ONE launch (its input refreshed outside the events: the state is
written back in place), the two arms alternating, medians over the windows after two warm-up
windows each.  At 1e3 rays that is what a launch costs on the queue, not a kernel's duration.
(--quick: fewer windows, no 1e7.)
"""

from __future__ import annotations

import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _forbes as F  # noqa: E402
from tests._util import load_case  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "forbes.txt")
TORCH = {np.float64: torch.float64, np.float32: torch.float32}


def disc_rays(n, radius, z0, tilt_deg, dtype, seed=7):
    """n collimated rays over a disc of `radius` at z0, tilted by tilt_deg about x."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = radius * torch.rand(n, generator=g, device=DEV, dtype=torch.float64).sqrt()
    th = 2 * np.pi * torch.rand(n, generator=g, device=DEV, dtype=torch.float64)
    m, c = np.sin(np.radians(tilt_deg)), np.cos(np.radians(tilt_deg))
    planes = [r * th.cos(), r * th.sin() + z0 * m / c, torch.full_like(r, z0),
              torch.zeros_like(r), torch.full_like(r, m), torch.full_like(r, c),
              torch.ones_like(r), torch.zeros_like(r)]
    return [p.to(TORCH[dtype]).contiguous() for p in planes]


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches   # ms


def main():
    from optiland_amd.engine import HipSystem

    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    assert torch.cuda.is_available(), "this measurement needs the GPU (no CPU figure stands in)"
    lines = [f"# tools/gpu_forbes.py{' --quick' if quick else ''} on {torch.cuda.get_device_name(0)}"]

    lines.append("\n## fixture cases: worst error / bound, per case (fp64, fp32)")
    worst = {np.float64: 0.0, np.float32: 0.0}
    for name in F.case_names():
        c = F.case(name)
        eng = HipSystem(c["table"], DEV)
        ratios = []
        for dtype in (np.float64, np.float32):
            rays = [torch.as_tensor(np.ascontiguousarray(p), dtype=TORCH[dtype], device=DEV)
                    for p in c["rows"][0]]
            eng.trace_forbes(rays, F.FORBES, 0, write_rays=True)
            got = np.stack([p.double().cpu().numpy() for p in rays])
            keep = ~c["edge"]
            err = np.nan_to_num(np.abs(got - c["rows"][F.FORBES]))[:, keep].max(axis=1)
            same_nan = np.array_equal(np.isnan(got), np.isnan(c["rows"][F.FORBES]))
            ratio = float((err / F.bound(c, dtype)[F.FORBES, :, 0]).max())
            worst[dtype] = max(worst[dtype], ratio)
            ratios.append(f"{ratio:.3g} (max {err.max():.2e}{'' if same_nan else ', NaN PATTERN DIFFERS'})")
        eng.close()
        lines.append(f"{name:22s} " + "   ".join(ratios))
    lines.append(f"worst ratio: fp64 {worst[np.float64]:.3g}, fp32 {worst[np.float32]:.3g}")

    lines.append("\n## one launch: ol_trace_forbes against ol_trace(first = last = s) on the even "
                 "asphere of aspheric_singlet\n"
                 "# kind dtype N | forbes ms  GB/s | asphere ms  GB/s | ratio forbes / asphere")
    asph_table, _ = load_case("aspheric_singlet")
    s_asph = int(np.nonzero(asph_table.surfaces["geom_kind"] == 2)[0][0])
    asph = HipSystem(asph_table, DEV)
    sizes = (1000, 100_000) if quick else (1000, 100_000, 10_000_000)
    for kind in F.KINDS:
        eng = HipSystem(F.case(f"{kind}_norm12_default")["table"], DEV)
        for dtype in (np.float32, np.float64):
            for n in sizes:
                windows = max(3, min(60, int(2e7 // n))) * (1 if quick else 2)
                src = (disc_rays(n, 9.0, -18.0, 2.5, dtype), disc_rays(n, 10.0, -20.0, 0.0, dtype))
                work = ([t.clone() for t in src[0]], [t.clone() for t in src[1]])
                stride = HipSystem.record_stride(n, np.dtype(dtype).itemsize)
                row = torch.empty((1, 8, stride), dtype=TORCH[dtype], device=DEV)

                def run_forbes():
                    eng.trace_forbes(work[0], F.FORBES, 0, record_row=row[0], write_rays=True,
                                     check_status=False)

                def run_asph():
                    asph.trace(work[1], 0, record=row, first=s_asph, last=s_asph, write_rays=True,
                               check_status=False)

                # The state is written back into the planes it was read from, so every timed
                # launch starts from a fresh copy of the source rays, made OUTSIDE the events:
                # one launch per window, the two arms alternating.
                runs, times = (run_forbes, run_asph), ([], [])
                for w in range(windows + 2):
                    for which in ((0, 1) if w % 2 == 0 else (1, 0)):
                        for dst, s_ in zip(work[which], src[which]):
                            dst.copy_(s_)
                        t = timed(runs[which], 1)
                        if w >= 2:   # (two warm-up windows per arm)
                            times[which].append(t)
                t_f, t_a = times
                mf, ma = statistics.median(t_f), statistics.median(t_a)
                size = 24 * n * np.dtype(dtype).itemsize
                lines.append(f"{kind:4s} {np.dtype(dtype).name:8s} {n:>9d} | {mf:9.4f} "
                             f"{size / mf / 1e6:8.1f} | {ma:9.4f} {size / ma / 1e6:8.1f} | "
                             f"{mf / ma:6.3f}   (spread forbes {min(t_f):.4f}-{max(t_f):.4f}, "
                             f"asphere {min(t_a):.4f}-{max(t_a):.4f})")
                print(lines[-1], flush=True)
        eng.close()
    asph.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
