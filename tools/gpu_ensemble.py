#!/usr/bin/env python
"""Measure the ensemble spot launch on the GPU (`ol_trace_spot_ensemble`) -> profiles/ensemble.txt.

    python tools/gpu_ensemble.py [--quick] [--out FILE] [--static FILE]

K = 64 / 128 / 256 / 1024 / 4096 variants of the Cooke triplet (the fixture's nominal table with one radius
drawn per variant from a seeded generator) x 3 fields x 91 and 1261 hexapolar rays at the primary
wavelength, fp32 and fp64, traced to spot moments in two ways that alternate in ONE process:

  ensemble   `SystemEnsemble.trace_spot`: the cells uploaded, ONE launch, one status read-back
             (the ensemble itself is built once, outside the window: a tolerancing run builds it
             once per batch of variants -- its build time is the last column; ensemble call +
             build against the loop is what a one-shot caller such as `monte_carlo_spots` sees)
  loop       what the same work costs without it: per variant `HipSystem.update` (the table
             re-written in place) + `trace_spot_batch` (the three fields in one launch) with its
             status read-back, K times

Per (K, rays, dtype): both times (host clock around the call, which ends in a device
synchronise: the read-back), their ratio, the time of the ensemble LAUNCH alone (device events
around the one launch, cells already on the device, no read-back) and its share of the call, and
the ray-surface rate of that launch (K x 3 x rays x 7 traced surfaces over the launch time).
Also checked at every size, before anything is timed: both arms give the same counts and their
moment sums agree to 1e-9 relative (reordered sums).
Times: medians over the windows after two warm-up windows per arm.  `--static FILE`: the text of
`tools/kernel_resources.py --filter ensemble_spot` (made where hipcc is) is appended.
(--quick: K = 64 and 256 only, fewer windows.)
"""

from __future__ import annotations

import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from optiland_amd.engine import HipSystem  # noqa: E402
from optiland_amd.ensemble import SystemEnsemble, cell_grid, pupil_points  # noqa: E402
from tests import _ensemble as E  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "ensemble.txt")
FIELDS = [(0.0, 0.0), (0.0, 0.7), (0.0, 1.0)]
TRACED = 7   # surfaces of the Cooke triplet a ray meets (6 lens surfaces + the image)


def variants(K, seed=1):
    base = E.tables("cooke")[0]
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        t = copy.deepcopy(base)
        t.surfaces["radius"][5] *= 1.0 + 1e-3 * rng.standard_normal()   # (behind the stop)
        out.append(t)
    return out


def main(argv):
    quick = "--quick" in argv
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else OUT
    static = argv[argv.index("--static") + 1] if "--static" in argv else None
    assert torch.cuda.is_available(), "tools/gpu_ensemble.py measures on the GPU"
    lines = [f"# ensemble spot launch vs a loop of update + trace_spot_batch, "
             f"{torch.cuda.get_device_name(0)}",
             "# Cooke triplet, 3 fields, primary wavelength; times in ms: median (min .. max)",
             f"# {'dtype':<5} {'K':>5} {'rays':>5}  {'ensemble call':>22}  {'loop':>26}  "
             f"{'loop/ens':>8}  {'launch':>8}  {'share':>6}  {'ray-surf/s':>10}  {'build':>8}"]
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        for K in ((64, 256) if quick else (64, 128, 256, 1024, 4096)):
            tabs = variants(K)
            SystemEnsemble(tabs[:2], DEV, dt).close()   # (first use of the library and the device)
            wl = tabs[0].reference_wavelength_index()
            t0 = time.perf_counter()
            ens = SystemEnsemble(tabs, DEV, dt)
            torch.cuda.synchronize()
            build_ms = (time.perf_counter() - t0) * 1e3
            hs = HipSystem(tabs[0], DEV)
            cells = cell_grid(K, FIELDS, [wl])
            loop_cells = [(hx, hy, 1.0, 1.0, 0.0, 0.0, wl) for hx, hy in FIELDS]
            for rings in (5, 20):
                x, y = pupil_points("hexapolar", rings)
                px = torch.from_numpy(x).to(DEV, dt)
                py = torch.from_numpy(y).to(DEV, dt)
                n = int(px.numel())

                def ensemble():
                    return ens.trace_spot(px, py, cells)[0]

                def loop():
                    outs = []
                    for t in tabs:
                        if not hs.update(t):
                            raise RuntimeError("HipSystem.update did not fit")
                        outs.append(hs.trace_spot_batch(px, py, loop_cells)[0])
                    return torch.stack(outs)

                a = ensemble().cpu().numpy().reshape(K, 3, 8)
                b = loop().cpu().numpy().reshape(K, 3, 8)
                assert np.array_equal(a[..., 0], b[..., 0]), "the two arms count differently"
                rel = np.abs(a[..., :6] - b[..., :6]).max() / np.abs(b[..., :6]).max()
                assert rel <= 1e-9, rel

                windows = 3 if quick else (9 if K <= 1024 else 5)
                # two warm-up windows per arm, then the arms alternate window by window
                et, lt = [], []
                for _ in range(2):
                    ensemble()
                    loop()
                for _ in range(windows):
                    for arm, acc in ((ensemble, et), (loop, lt)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        arm()
                        torch.cuda.synchronize()
                        acc.append((time.perf_counter() - t0) * 1e3)
                e_ms, l_ms = statistics.median(et), statistics.median(lt)

                cells_dev = torch.from_numpy(
                    np.ascontiguousarray(cells.reshape(-1)).view(np.uint8)).to(DEV)
                out8 = torch.zeros((K * 3, 8), dtype=torch.float64, device=DEV)
                ev = []
                for _ in range(3 + 2 * windows):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    ens.trace_spot(px, py, cells_dev, out=out8, check_status=False)
                    e.record()
                    torch.cuda.synchronize()
                    ev.append(s.elapsed_time(e))
                k_ms = statistics.median(ev[3:])
                rate = K * 3 * n * TRACED / (k_ms * 1e-3)
                lines.append(
                    f"  {tag:<5} {K:>5} {n:>5}  {e_ms:>8.3f} ({min(et):.3f} .. {max(et):.3f})  "
                    f"{l_ms:>9.2f} ({min(lt):.2f} .. {max(lt):.2f})  {l_ms / e_ms:>8.1f}  "
                    f"{k_ms:>8.4f}  {100 * k_ms / e_ms:>5.1f}%  {rate:>10.3g}  {build_ms:>8.1f}")
                print(lines[-1], flush=True)
            ens.close()
            hs.close()
    if static and os.path.exists(static):
        lines += ["", "# static resources of the ensemble kernels (tools/kernel_resources.py "
                      "--filter ensemble_spot):"]
        lines += [ln.rstrip("\n") for ln in open(static)]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
