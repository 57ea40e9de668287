#!/usr/bin/env python
"""Measure the phase-surface one-surface launch on the GPU (`ol_trace_phase`) -> profiles/phase.txt.

    python tools/gpu_phase.py [--quick] [--out FILE]

* the worst error of every fixture case (tests/golden/phase.npz) as a share of its bound
  (tests/_phase.py), fp64 and fp32, and fp64 against the 1e-12 bound;
* the time of one `ol_trace_phase` launch at N = 1e3, 1e5 and 1e7 rays, fp32 and fp64, on the
  radial, the linear and the grid row (24 x 18 nodes, and the same plane with 512 x 512 nodes),
  recording a row and writing the state back: 8 planes read, 16 written, plus the four gathers of
  a grid row (not counted in the bytes);
* beside each, the existing one-surface launch `ol_trace(first = last = s)` on a standard surface
  of double_gauss at the same N and dtype with the same traffic, measured TWICE (arms A and B):
  the spread between the two is the margin a ratio is read against;
* bytes moved per second (24 planes x N x element size over the time);
* end to end, only where the reference package is present: `Optic.trace` of the radial metalens
  and of the grid optic of tests/_phase.py under `enable()` at 1e3, 1e5 and 1e6 rays, with the
  device kernel and with `enable(phases=False)` (what OPTILAND_HIP_PHASES=0 sets: the reference's
  own surface, the behaviour before this kernel), alternating in one process.
Times: device events around ONE launch (its input refreshed outside the events: the state is
written back in place), the arms alternating, medians over the windows after two warm-up windows
each.  At 1e3 rays that is what a launch costs on the queue, not a kernel's duration.
(--quick: fewer windows, no 1e7, no 1e6.)
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

from optiland_amd import system as S  # noqa: E402
from tests import _live  # noqa: E402
from tests import _phase as P  # noqa: E402
from tests._util import load_case  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "phase.txt")
TORCH = {np.float64: torch.float64, np.float32: torch.float32}


def disc_rays(n, radius, z0, tilt_deg, dtype, seed=7):
    """n collimated rays over a disc of `radius` at z0, tilted by tilt_deg about x."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = radius * torch.rand(n, generator=g, device=DEV, dtype=torch.float64).sqrt()
    th = 2 * np.pi * torch.rand(n, generator=g, device=DEV, dtype=torch.float64)
    m, c = np.sin(np.radians(tilt_deg)), np.cos(np.radians(tilt_deg))
    planes = [r * th.cos(), r * th.sin(), torch.full_like(r, z0),
              torch.zeros_like(r), torch.full_like(r, m), torch.full_like(r, c),
              torch.ones_like(r), torch.zeros_like(r)]
    return [p.to(TORCH[dtype]).contiguous() for p in planes]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)   # ms


def big_grid_table(nodes_per_axis=512):
    """The grid case's table with the same plane sampled at nodes_per_axis^2 nodes."""
    t = S.SystemTable.from_json(P.case("grid")["table"].to_json())
    g = P.PHASE
    off, n = int(t.surfaces["coeff_offset"][g]), int(t.surfaces["n_coeff"][g])
    assert off + n == t.coeffs.size
    xs = np.linspace(P.GRID_X[0], P.GRID_X[1], nodes_per_axis)
    ys = np.linspace(P.GRID_Y[0], P.GRID_Y[1], nodes_per_axis)
    block = np.concatenate([[float(S.PHASE_GRID), 1.0, nodes_per_axis, nodes_per_axis, xs[0],
                             xs[-1], ys[0], ys[-1], 0.0],
                            P.radial_phase(xs[None, :], ys[:, None]).reshape(-1)])
    t.coeffs = np.concatenate([t.coeffs[:off], block])
    t.surfaces["n_coeff"][g] = block.size
    for later in range(g + 1, t.surfaces.shape[0]):   # (rows without a block point at the end)
        assert int(t.surfaces["n_coeff"][later]) == 0
        t.surfaces["coeff_offset"][later] = t.coeffs.size
    return t


def errors(lines):
    from optiland_amd.engine import HipSystem

    lines.append("\n## fixture cases: worst error / bound (fp64 contract, fp64 at 1e-12, fp32 contract)")
    worst = [0.0, 0.0, 0.0]
    for name in P.case_names():
        c = P.case(name)
        g, wl = c["g"], c["wl"]
        eng = HipSystem(c["table"], DEV)
        scale = P.scale_of(c["rows"][:g + 1])
        out = []
        for k, (dtype, tight) in enumerate(((np.float64, False), (np.float64, True),
                                            (np.float32, False))):
            rays = [torch.as_tensor(np.array(p), dtype=TORCH[dtype], device=DEV)
                    for p in c["rows"][g - 1]]
            eng.trace_phase(rays, g, wl, write_rays=True)
            got = np.stack([p.double().cpu().numpy() for p in rays])
            want = c["rows"][g]
            same = np.array_equal(np.isnan(got), np.isnan(want)) and \
                np.array_equal(got[6] == 0, want[6] == 0)
            err = np.nan_to_num(np.abs(got - want)) / P.bounds(dtype, scale, tight)
            worst[k] = max(worst[k], float(err.max()))
            out.append(f"{float(err.max()):.3g}{'' if same else ' MASK DIFFERS'}")
        eng.close()
        lines.append(f"{name:14s} " + "   ".join(out))
    lines.append(f"worst: fp64 {worst[0]:.3g}, fp64 at 1e-12 {worst[1]:.3g}, fp32 {worst[2]:.3g}")


def launches(lines, quick):
    from optiland_amd.engine import HipSystem

    lines.append("\n## one launch: ol_trace_phase against ol_trace(first = last = s) on a standard "
                 "surface of double_gauss (arms A and B: the same launch twice)\n"
                 "# row dtype N | phase ms  TB/s | A ms  B ms  TB/s(A) | phase / A | spread |A - B| / A")
    dg_table, _ = load_case("double_gauss")
    rows = dg_table.surfaces
    s_std = next(i for i in range(1, len(rows)) if int(rows["geom_kind"][i]) == 1
                 and np.isfinite(rows["radius"][i]) and int(rows["interaction"][i]) == 1)
    z_std = float(rows["origin"][s_std][2])
    base = HipSystem(dg_table, DEV)
    sizes = (1000, 100_000) if quick else (1000, 100_000, 10_000_000)
    tables = (("radial", P.case("radial_t")["table"]), ("linear", P.case("linear_m1")["table"]),
              ("grid24x18", P.case("grid")["table"]), ("grid512^2", big_grid_table()))
    for kind, table in tables:
        g = P.PHASE
        z_g = float(table.surfaces["origin"][g][2])
        eng = HipSystem(table, DEV)
        for dtype in (np.float32, np.float64):
            for n in sizes:
                windows = max(3, min(60, int(2e7 // n))) * (1 if quick else 2)
                src = (disc_rays(n, 3.0, z_g - 2.0, 4.0, dtype),
                       disc_rays(n, 5.0, z_std - 2.0, 2.0, dtype))
                work = ([t.clone() for t in src[0]], [t.clone() for t in src[1]])
                stride = HipSystem.record_stride(n, np.dtype(dtype).itemsize)
                row = torch.empty((1, 8, stride), dtype=TORCH[dtype], device=DEV)

                def run_phase():
                    eng.trace_phase(work[0], g, 0, record_row=row[0], write_rays=True,
                                    check_status=False)

                def run_base():
                    base.trace(work[1], 0, record=row, first=s_std, last=s_std, write_rays=True,
                               check_status=False)

                arms = ((run_phase, 0), (run_base, 1), (run_base, 1))   # phase, A, B
                times = ([], [], [])
                for w in range(windows + 2):
                    order = (0, 1, 2) if w % 2 == 0 else (2, 1, 0)
                    for k in order:
                        fn, which = arms[k]
                        for dst, s_ in zip(work[which], src[which]):
                            dst.copy_(s_)
                        t = timed(fn)
                        if w >= 2:
                            times[k].append(t)
                mg, ma, mb = (statistics.median(t) for t in times)
                size = 24 * n * np.dtype(dtype).itemsize
                lines.append(f"{kind:10s} {np.dtype(dtype).name:8s} {n:>9d} | {mg:9.4f} "
                             f"{size / mg / 1e9:7.3f} | {ma:9.4f} {mb:9.4f} {size / ma / 1e9:7.3f} | "
                             f"{mg / ma:6.3f} | {abs(ma - mb) / ma:6.3f}   (phase "
                             f"{min(times[0]):.4f}-{max(times[0]):.4f})")
                print(lines[-1], flush=True)
        eng.close()
    base.close()


def end_to_end(lines, quick):
    if _live.reference_root() is None:
        lines.append("\n## end to end: the reference package is not present here -- leg skipped")
        return
    be = _live.import_reference()
    from optiland_amd import integration as I

    be.set_backend("torch")
    be.set_device("cuda")
    be.set_precision("float64")
    lines.append("\n## end to end: Optic.trace of the metalens of tests/_phase.py under enable(), "
                 "torch backend on the device, fp64\n"
                 "# optic N | device kernel ms | reference's surface ms (enable(phases=False)) | "
                 "factor | foreign surfaces with the kernel")
    try:
        for kind in ("radial", "grid"):
            lens = P.lens(kind, material="N-BK7")
            for n in (1000, 100_000) if quick else (1000, 100_000, 1_000_000):
                times = {True: [], False: []}
                reps = 3 if n >= 1_000_000 else 7
                foreign = 0
                for w in range(reps + 1):
                    for on in ((True, False) if w % 2 == 0 else (False, True)):
                        I.enable(phases=on)
                        before = I._SG["foreign"]
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        lens.trace(0.0, 1.0, P.WAVELENGTH, n, "random")
                        torch.cuda.synchronize()
                        if w >= 1:
                            times[on].append((time.perf_counter() - t0) * 1e3)
                        if on:
                            foreign += I._SG["foreign"] - before
                a, b = statistics.median(times[True]), statistics.median(times[False])
                lines.append(f"{kind:7s} {n:>9d} | {a:10.3f} | {b:10.3f} | {b / a:6.2f} x | "
                             f"{foreign}")
                print(lines[-1], flush=True)
    finally:
        I.enable(phases=True)
        I.disable()
        be.set_backend("numpy")


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    assert torch.cuda.is_available(), "this measurement needs the GPU (no CPU figure stands in)"
    lines = [f"# tools/gpu_phase.py{' --quick' if quick else ''} on {torch.cuda.get_device_name(0)}"]
    errors(lines)
    launches(lines, quick)
    end_to_end(lines, quick)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
