#!/usr/bin/env python
"""Measure the ensemble wavefront call on the GPU (`ol_trace_opd_ensemble`)
-> profiles/ensemble_opd.txt.

    python tools/gpu_ensemble_opd.py [--quick] [--out FILE] [--static FILE]

K = 64 / 128 / 256 / 1024 / 4096 variants of the Cooke triplet (the fixture's nominal table with
one radius drawn per variant from a seeded generator) x 3 fields x 91 and 469 hexapolar rays at
the primary wavelength, fp64, taken to OPD moments in two ways that alternate in ONE process:

  ensemble   `SystemEnsemble.trace_opd`: the cells uploaded, the chief-ray launch and the OPD
             launch, one status read-back (the ensemble itself is built once, outside the
             window; its build time is the last column -- build + call against the loop is what
             a one-shot caller such as `tolerancing.monte_carlo` sees)
  loop       what the same work costs without it: per variant `HipSystem.update`, then per field
             `wavefront_reference` + `trace_opd(reference=)` with its status read-back

Per (K, rays): both times (host clock around the call, which ends in a device synchronise), their
ratio, the time of the two ensemble LAUNCHES alone (device events, cells already on the device, no
read-back) and, as an upper bound of the chief-ray launch's share of them, the same two launches
with ONE ray per cell.  Checked at every size before anything is timed: both arms count the same
rays and their moment sums agree to 1e-9 relative.  Also recorded: how far the ensemble's OPD is
from the single launches' off axis, against what one ulp of the field moves the single launches
(the bound of tests/test_gpu_ensemble_opd.py).

Every size runs in a child process of its own under `timeout`; the first one that fails ends the
run.  Times: medians over the windows after two warm-up windows per arm, with the spread.
`--static FILE`: the text of `tools/kernel_resources.py --filter opd` (made where hipcc is) is
appended.  (--quick: K = 64 and 256 only, fewer windows.)
"""

from __future__ import annotations

import copy
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "ensemble_opd.txt")
FIELDS = [(0.0, 0.0), (0.0, 0.7), (0.0, 1.0)]
SIZES, QUICK = (64, 128, 256, 1024, 4096), (64, 256)
RINGS = (5, 12)      # 91 and 469 hexapolar points
DEV = "cuda:0"


def variants(K, seed=1):
    import numpy as np

    from tests import _ensemble_opd as EO
    base = EO.tables("cooke")[0]
    rng = np.random.default_rng(seed)
    out = []
    for _k in range(K):
        t = copy.deepcopy(base)
        t.surfaces["radius"][5] *= 1.0 + 1e-3 * rng.standard_normal()   # (behind the stop)
        out.append(t)
    return out


def one_size(K: int, quick: bool) -> list:
    import numpy as np
    import torch

    from optiland_amd.analysis_seams import _launch_plane_tilt
    from optiland_amd.engine import HipSystem
    from optiland_amd.ensemble import SystemEnsemble, opd_cell_grid, pupil_points
    tabs = variants(K)
    SystemEnsemble(tabs[:2], DEV, torch.float64).close()   # (first use of library and device)
    wl = tabs[0].reference_wavelength_index()
    t0 = time.perf_counter()
    ens = SystemEnsemble(tabs, DEV, torch.float64)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    hs = HipSystem(tabs[0], DEV)
    cells = opd_cell_grid(tabs, FIELDS, [wl])
    lines = []
    for rings in RINGS:
        x, y = pupil_points("hexapolar", rings)
        px, py = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
        n = int(px.numel())

        def ensemble():
            return ens.trace_opd(px, py, cells)[0]

        def loop():
            outs = []
            for t in tabs:
                if not hs.update(t):
                    raise RuntimeError("HipSystem.update did not fit")
                rg = t.raygen
                for hx, hy in FIELDS:
                    ux, uy = _launch_plane_tilt(rg, hx, hy)
                    params = dict(n_image=rg["n_image"], ux=ux, uy=uy, half_epd=rg["EPD"] / 2.0,
                                  wavelength_um=float(t.wavelengths[wl]),
                                  last_thickness=float(t.last_thickness))
                    ref, _c = hs.wavefront_reference(params, wl, field=(hx, hy),
                                                     pupil_z=rg["pupil_z"])
                    outs.append(hs.trace_opd(None, px, py, wl, field=(hx, hy), want_pupil=False,
                                             reference=ref)[3])
            return torch.stack(outs)

        a = ensemble().cpu().numpy()
        b = loop().cpu().numpy()
        assert np.array_equal(a[:, 9], b[:, 9]), "the two arms count differently"
        rel = np.abs(a - b).max() / np.abs(b).max()
        assert rel <= 1e-9, rel

        windows = 3 if quick else (9 if K <= 1024 else 5)
        et, lt = [], []
        for _ in range(2):     # two warm-up windows per arm, then the arms alternate
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

        cells_dev = torch.from_numpy(np.ascontiguousarray(cells.reshape(-1)).view(np.uint8)).to(DEV)
        mom = torch.zeros((K * 3, 12), dtype=torch.float64, device=DEV)
        refs = torch.zeros((K * 3, 16), dtype=torch.float64, device=DEV)

        def launches(qx, qy):
            ev = []
            for _ in range(3 + 2 * windows):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                ens.trace_opd(qx, qy, cells_dev, out=mom, refs=refs, check_status=False)
                e.record()
                torch.cuda.synchronize()
                ev.append(s.elapsed_time(e))
            return statistics.median(ev[3:])

        k_ms, chief_ms = launches(px, py), launches(px[:1], py[:1])
        lines.append(
            f"  {K:>5} {n:>5}  {e_ms:>8.3f} ({min(et):.3f} .. {max(et):.3f})  "
            f"{l_ms:>9.2f} ({min(lt):.2f} .. {max(lt):.2f})  {l_ms / e_ms:>8.1f}  "
            f"{k_ms:>8.4f}  {chief_ms:>8.4f}  {100 * chief_ms / k_ms:>5.1f}%  {build_ms:>8.1f}")
    ens.close()
    hs.close()
    return lines


def ulp_lines() -> list:
    """The off-axis bound of tests/test_gpu_ensemble_opd.py on the fixture's Cooke cells."""
    import numpy as np
    import torch

    from optiland_amd.engine import HipSystem
    from tests import _ensemble_opd as EO
    from tests import test_gpu_ensemble_opd as T
    lines = []
    for lens in ("cooke", "singlet"):
        tabs, a, _cells, _mom, _refs, planes = T.launch(lens)
        px, py = T._t(a["px"]), T._t(a["py"])
        moved = diff = 0.0
        for k, t in enumerate(tabs):
            hs = HipSystem(t, DEV)
            (hx, hy), fi = a["fields"][1], 1
            for wi, w in enumerate(EO.wavelength_indices(lens, tabs[0])):
                _r, pl, _m = T.single(hs, t, (hx, hy), w, px, py)
                lit = pl[1] > 0
                diff = max(diff, float(np.abs(planes[k, fi, wi, 0] - pl[0])[lit].max()))
                for step in (np.inf, -np.inf):
                    _r, p2, _m = T.single(hs, t, (hx, np.nextafter(hy, step)), w, px, py)
                    moved = max(moved, float(np.abs(p2[0] - pl[0])[lit].max()))
            hs.close()
        lines.append(f"#   {lens}: ensemble against single launches {diff:.3e} waves, single "
                     f"launches under one ulp of hy {moved:.3e} waves, ratio {diff / moved:.3f} "
                     f"(bound 4)")
    torch.cuda.synchronize()
    return lines


def main(argv):
    if "--one" in argv:      # a child: one size, its lines on stdout
        import torch
        assert torch.cuda.is_available(), "tools/gpu_ensemble_opd.py measures on the GPU"
        what = argv[argv.index("--one") + 1]
        lines = [f"# {torch.cuda.get_device_name(0)}"] + ulp_lines() if what == "ulp" \
            else one_size(int(what), "--quick" in argv)
        print("\n".join("@" + ln for ln in lines), flush=True)
        return 0
    quick = "--quick" in argv
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else OUT
    static = argv[argv.index("--static") + 1] if "--static" in argv else None
    lines = ["# ensemble wavefront call vs a loop of update + wavefront_reference + trace_opd, "
             "fp64",
             "# Cooke triplet, 3 fields, primary wavelength; times in ms: median (min .. max)",
             "# `1 ray`: the two launches with one ray per cell -- the chief-ray launch and an OPD "
             "launch of one ray: an upper bound of the chief launch's share of `launches`",
             f"# {'K':>5} {'rays':>5}  {'ensemble call':>22}  {'loop':>26}  {'loop/ens':>8}  "
             f"{'launches':>8}  {'1 ray':>8}  {'share':>6}  {'build':>8}"]
    steps = [(str(K), 60 + K // 8) for K in (QUICK if quick else SIZES)] + [("ulp", 120)]
    for what, limit in steps:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
               "--one", what] + (["--quick"] if quick else [])
        p = subprocess.run(cmd, capture_output=True, text=True)
        got = [ln[1:] for ln in p.stdout.splitlines() if ln.startswith("@")]
        if what == "ulp":
            lines += ["", "# off axis, the fixture's cells at field 0.7 "
                          "(tests/test_gpu_ensemble_opd.py):"]
        lines += got
        print("\n".join(got), flush=True)
        if p.returncode:     # nothing more is started on the GPU after a step that failed,
            sys.stderr.write(p.stderr[-4000:])     # and no earlier measurement is overwritten
            print(f"step {what} ended with status {p.returncode}: the run stops here, "
                  f"{out_path} is left as it was")
            return 1
    if static and os.path.exists(static):
        lines += ["", "# static resources of the OPD kernels (tools/kernel_resources.py --filter "
                      "opd):"]
        lines += [ln.rstrip("\n") for ln in open(static)]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
