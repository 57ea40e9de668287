#!/usr/bin/env python
"""Measure the grid-sag one-surface launch on the GPU (`ol_trace_grid_sag`) -> profiles/grid_sag.txt.

    python tools/gpu_grid_sag.py [--quick] [--out FILE]

* the worst error of every fixture case (tests/golden/grid_sag.npz) as a share of its bound
  (tests/_grid_sag.py): fp64 at tol = 1e-12 against 1e-12, fp64 and fp32 at the factory tolerance
  against the contract; and the device against the host run of the same source (fp64), where the
  host checker can be built;
* the time of one `ol_trace_grid_sag` launch at N = 1e3, 1e5 and 1e7 rays, fp32 and fp64, on the
  33 x 29 grid of the fixture and on the same surface sampled at 512 x 512 nodes, recording a row
  and writing the state back: 8 planes read, 16 written, plus per Newton pass two coordinate pairs
  and four nodes per ray (not counted in the bytes);
* beside each, the existing one-surface launch `ol_trace(first = last = s)` on the even-asphere
  surface of aspheric_singlet at the same N and dtype with the same plane traffic, measured TWICE
  (arms A and B): the spread between the two is the margin a ratio is read against;
* bytes moved per second (24 planes x N x element size over the time);
* end to end, only where the reference package is present: `Optic.trace` of the singlet of
  tests/_grid_sag.py under `enable()` at 1e3, 1e5 and 1e6 rays, with the device kernel and with
  `enable(grid_sags=False)` (the reference's own surface, the behaviour before this kernel),
  alternating in one process; the same with a grid narrower than the beam, where one NaN ray has
  the reference run all its 100 passes.
* the static resources of the two kernels (tools/kernel_resources.py's compile of grid_sag.hip
  with the product's flags: VGPRs, SGPRs, spills, scratch, waves per SIMD), where hipcc is present.
How to read the figures -- which limiter binds at which size -- is in DESIGN.md ("Grid-sag
surfaces") and the README, not in the file this tool writes.
Times: device events around ONE launch (its input refreshed outside the events: the state is
written back in place), the arms alternating, medians over the windows after two warm-up windows
each.  At 1e3 rays that is what a launch costs on the queue, not a kernel's duration.
(--quick: fewer windows, no 1e7, no 1e6.)
"""

from __future__ import annotations

import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from optiland_amd import system as S  # noqa: E402
from tests import _grid_sag as G  # noqa: E402
from tests import _live  # noqa: E402
from tests._util import load_case  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "grid_sag.txt")
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


def resampled_table(nodes_per_axis=512):
    """The uniform case's table with the same surface sampled at nodes_per_axis^2 nodes."""
    t = S.SystemTable.from_json(G.case("uniform", "factory")["table"].to_json())
    g = G.GRID
    off, n = int(t.surfaces["coeff_offset"][g]), int(t.surfaces["n_coeff"][g])
    assert off + n == t.coeffs.size
    xs = ys = G.axis(8.0, nodes_per_axis)
    block = np.concatenate([[float(xs.size), float(ys.size)], xs, ys,
                            G.sag_table(xs, ys, 30.0).reshape(-1)])
    t.coeffs = np.concatenate([t.coeffs[:off], block])
    t.surfaces["n_coeff"][g] = block.size
    for later in range(g + 1, t.surfaces.shape[0]):   # (rows without a block point at the end)
        assert int(t.surfaces["n_coeff"][later]) == 0
        t.surfaces["coeff_offset"][later] = t.coeffs.size
    return t


def errors(lines):
    from optiland_amd.engine import HipSystem

    lines.append("\n## fixture cases: worst error / bound (fp64 at tol 1e-12 against 1e-12; fp64, "
                 "fp32 at tol 1e-6 against the contract) and device against host run (fp64, share "
                 "of the plane's scale)")
    b = G._builder()
    exe = b.build() if b.available() else None
    tmp = tempfile.mkdtemp()
    worst = [0.0, 0.0, 0.0, 0.0]
    for name in G.case_names():
        out = []
        for k, (tol, dtype, tight) in enumerate((("tight", np.float64, True),
                                                 ("factory", np.float64, False),
                                                 ("factory", np.float32, False))):
            c = G.case(name, tol)
            eng = HipSystem(c["table"], DEV)
            rays = [torch.as_tensor(np.array(p), dtype=TORCH[dtype], device=DEV)
                    for p in c["before"]]
            eng.trace_grid_sag(rays, G.GRID, 0, write_rays=True, check_status=False)
            got = np.stack([p.double().cpu().numpy() for p in rays])
            eng.close()
            want = c["after"]
            same = np.array_equal(np.isnan(got), np.isnan(want)) and \
                np.array_equal(got[6] == 0, want[6] == 0)
            scale = G.scale_of(np.stack([c["before"], c["after"], c["lens"]]))
            err = np.nan_to_num(np.abs(got - want)) / G.bounds(dtype, scale, tight)
            worst[k] = max(worst[k], float(err.max()))
            out.append(f"{float(err.max()):.3g}{'' if same else ' MASK DIFFERS'}")
            if k == 0 and exe is not None:
                path = os.path.join(tmp, "host.case")
                G.write_case(path, c["table"], c["before"])
                host, _bits = G.host_step(exe, path)
                span = np.maximum(1.0, np.nanmax(np.abs(host), axis=1, keepdims=True))
                dh = float(np.nan_to_num(np.abs(got - host) / span).max())
                worst[3] = max(worst[3], dh)
                out.append(f"host {dh:.3g}")
        lines.append(f"{name:12s} " + "   ".join(out))
    lines.append(f"worst: fp64 at 1e-12 {worst[0]:.3g}, fp64 {worst[1]:.3g}, fp32 {worst[2]:.3g}, "
                 f"device against host {worst[3]:.3g}")


def launches(lines, quick):
    from optiland_amd.engine import HipSystem

    lines.append("\n## one launch: ol_trace_grid_sag against ol_trace(first = last = s) on the even "
                 "asphere of aspheric_singlet (arms A and B: the same launch twice)\n"
                 "# grid dtype N | grid-sag ms  TB/s | A ms  B ms  TB/s(A) | grid-sag / A | spread "
                 "|A - B| / A")
    asph_table, _ = load_case("aspheric_singlet")
    s_asph = int(np.nonzero(asph_table.surfaces["geom_kind"] == 2)[0][0])
    z_asph = float(asph_table.surfaces["origin"][s_asph][2])
    base = HipSystem(asph_table, DEV)
    sizes = (1000, 100_000) if quick else (1000, 100_000, 10_000_000)
    tables = (("33x29", G.case("uniform", "factory")["table"]), ("512^2", resampled_table()))
    for kind, table in tables:
        g = G.GRID
        z_g = float(table.surfaces["origin"][g][2])
        eng = HipSystem(table, DEV)
        for dtype in (np.float32, np.float64):
            for n in sizes:
                windows = max(3, min(60, int(2e7 // n))) * (1 if quick else 2)
                src = (disc_rays(n, 5.0, z_g - 5.0, 2.0, dtype),
                       disc_rays(n, 3.0, z_asph - 2.0, 2.0, dtype))
                work = ([t.clone() for t in src[0]], [t.clone() for t in src[1]])
                stride = HipSystem.record_stride(n, np.dtype(dtype).itemsize)
                row = torch.empty((1, 8, stride), dtype=TORCH[dtype], device=DEV)

                def run_grid():
                    eng.trace_grid_sag(work[0], g, 0, record_row=row[0], write_rays=True,
                                       check_status=False)

                def run_base():
                    base.trace(work[1], 0, record=row, first=s_asph, last=s_asph, write_rays=True,
                               check_status=False)

                arms = ((run_grid, 0), (run_base, 1), (run_base, 1))   # grid-sag, A, B
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
                lines.append(f"{kind:6s} {np.dtype(dtype).name:8s} {n:>9d} | {mg:9.4f} "
                             f"{size / mg / 1e9:7.3f} | {ma:9.4f} {mb:9.4f} {size / ma / 1e9:7.3f} | "
                             f"{mg / ma:6.3f} | {abs(ma - mb) / ma:6.3f}   (grid-sag "
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
    lines.append("\n## end to end: Optic.trace of the singlet of tests/_grid_sag.py under enable(), "
                 "torch backend on the device, fp64, factory tolerance\n"
                 "# grid N | device kernel ms | reference's surface ms (enable(grid_sags=False)) | "
                 "factor | foreign surfaces with the kernel")
    try:
        for kind, edit in (("wide", {}), ("narrow", dict(half=4.6))):
            lens = G.lens(**edit)
            for n in (1000, 100_000) if quick else (1000, 100_000, 1_000_000):
                times = {True: [], False: []}
                reps = 3 if n >= 1_000_000 else 5
                foreign = 0
                for w in range(reps + 1):
                    for on in ((True, False) if w % 2 == 0 else (False, True)):
                        I.enable(grid_sags=on)
                        before = I._SG["foreign"]
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        lens.trace(0.0, 1.0, G.WAVELENGTH, n, "random")
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
        I.enable(grid_sags=True)
        I.disable()
        be.set_backend("numpy")


def resources(lines):
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "_kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    lines.append("\n## static resources of grid_sag.hip (tools/kernel_resources.py: gfx950, "
                 "product flags)\n"
                 f"# {'kernel':<40} {'VGPR':>5} {'SGPR':>5} {'sSpill':>6} {'vSpill':>6} "
                 f"{'scratch':>7} {'waves':>5} {'LDS':>5}")
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        lines.append("hipcc is not present here -- leg skipped")
        return
    rows = kr.parse(kr.compile_one("grid_sag.hip", []))
    for r, n in sorted(zip(rows, kr.demangle([r["name"] for r in rows])), key=lambda x: x[1]):
        lines.append(f"  {n:<40} {r.get('VGPRs', '?'):>5} {r.get('TotalSGPRs', '?'):>5} "
                     f"{r.get('SGPRs Spill', '?'):>6} {r.get('VGPRs Spill', '?'):>6} "
                     f"{r.get('ScratchSize [bytes/lane]', '?'):>7} "
                     f"{r.get('Occupancy [waves/SIMD]', '?'):>5} "
                     f"{r.get('LDS Size [bytes/block]', '?'):>5}")


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    assert torch.cuda.is_available(), "this measurement needs the GPU (no CPU figure stands in)"
    lines = [f"# tools/gpu_grid_sag.py{' --quick' if quick else ''} on "
             f"{torch.cuda.get_device_name(0)}"]
    errors(lines)
    launches(lines, quick)
    end_to_end(lines, quick)
    resources(lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
