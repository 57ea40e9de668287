"""The reference's Monte Carlo tolerancing loop as ONE ensemble launch (a function a user calls;
nothing of the reference is patched).

`MonteCarlo.run` (tolerancing/monte_carlo.py:60-123) does, per iteration: `tolerancing.reset()`,
every `perturbation.apply()`, the compensators, then every operand -- each `rms_spot_size` operand
one `Optic.trace` of a few hundred rays.  `monte_carlo_spots` replays exactly that order (so the
sampler draws are the reference's own), packs one table per iteration, builds a `SystemEnsemble`
of the iterations and evaluates every operand of every iteration in one
`ol_trace_spot_ensemble` launch.

The operand (optimization/operand/ray.py:336-340) is an UNMASKED mean over all rays; the device
moments are over the rays that arrive (intensity > 0).  Where a cell lost no ray the value follows
from its moments; where it did, it is computed from the cell's hits exactly as the operand
computes it -- clipped rays included, NaN included.

`monte_carlo` is the same replay for problems that also hold `OPD_difference` operands
(optimization/operand/ray.py:343-389: a `Wavefront` per operand, reduced to a mean absolute
deviation): every cell of a group of such operands goes in one `SystemEnsemble.trace_opd` call
(`ol_trace_opd_ensemble`) and the value is formed on the host from the cell's OPD plane.
"""

from __future__ import annotations

import numpy as np

from .ensemble import (StructureMismatch, SystemEnsemble, UnsupportedStructure, cell_grid,
                       check_structure, pupil_points, rms_about_centroid)
from .packer import UnsupportedSystem, pack_ensemble, pack_optic

# Below this many iterations `monte_carlo_spots` traces variant by variant (`HipSystem.update` +
# `trace_spot_batch`, the loop every caller ran before the ensemble existed) instead of building an
# ensemble.  Measured on the MI355X (profiles/ensemble.txt, tools/gpu_ensemble.py, 3 fields): the
# ensemble CALL is 33-39 x ahead of the loop at K = 64 (0.11 against 4.0 ms) and up to 600 x at
# K = 4096, but this function also BUILDS the ensemble, once (20-27 us per variant of host
# staging against the loop's ~63 us per variant).  Build + call against the loop: 5.9-9.2 against
# 4.0 ms at K = 64 (the loop ahead), 2.8 against 8.1 ms at K = 128, 5.6 against 16.4 at 256, 19.5
# against 62-66 at 1024, 95-111 against 251-268 at 4096 (the ensemble 2.3-3.2 x ahead).  The
# crossover lies between the measured 64 and 128; the constant is the first size measured ahead.
ENSEMBLE_MIN_VARIANTS = 128


def _operand_cells(tolerancing):
    """[(Hx, Hy, wavelength, num_rays, distribution)] of the problem's operands, or
    UnsupportedSystem."""
    optic = tolerancing.optic
    last = len(optic.surfaces.surfaces) - 1
    cells = []
    if getattr(tolerancing.compensator, "has_variables", False):
        raise UnsupportedSystem("monte_carlo_spots: compensators are not traced inside the launch")
    if not tolerancing.operands:
        raise ValueError("No operands found in the tolerancing system.")    # MonteCarlo._validate
    if not tolerancing.perturbations:
        raise ValueError("No perturbations found in the tolerancing system.")
    for i, op in enumerate(tolerancing.operands):
        if op.operand_type != "rms_spot_size":
            raise UnsupportedSystem(f"monte_carlo_spots: operand {i} is {op.operand_type!r}, not "
                                    f"'rms_spot_size'")
        d = dict(op.input_data)
        if d.get("optic") is not optic:
            raise UnsupportedSystem(f"monte_carlo_spots: operand {i} reads another optic")
        if isinstance(d.get("wavelength"), str):
            raise UnsupportedSystem(f"monte_carlo_spots: operand {i} has wavelength="
                                    f"{d['wavelength']!r} (one wavelength per operand)")
        s = int(d["surface_number"])
        if s not in (-1, last):
            raise UnsupportedSystem(f"monte_carlo_spots: operand {i} reads surface {s}, not the "
                                    f"image surface")
        cells.append((float(d["Hx"]), float(d["Hy"]), float(d["wavelength"]), int(d["num_rays"]),
                      str(d.get("distribution", "hexapolar"))))
    return cells


def operand_from_hits(x, y) -> float:
    """`RayOperand.rms_spot_size` on image-plane hits: sqrt(mean((x - mean x)^2 + (y - mean y)^2))
    over ALL rays."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.sqrt(np.mean((x - np.mean(x)) ** 2 + (y - np.mean(y)) ** 2)))


def monte_carlo_spots(tolerancing, num_iterations: int, device=None, dtype=None,
                      min_ensemble: int = ENSEMBLE_MIN_VARIANTS) -> list:
    """`MonteCarlo(tolerancing).run(num_iterations)` for problems whose operands are all
    `rms_spot_size` at one wavelength each and which have no compensators.  Returns one dict per
    iteration, keyed like the rows of the reference's results: the perturbation values under
    `str(perturbation.variable)`, then one value per operand under `f"{i}: {operand}"`.

    Raises `UnsupportedSystem` -- before anything is perturbed -- for compensators, operands of
    another type, `wavelength="all"` and an optic that fails strict packing.  Whether a
    perturbation changes a surface's KIND is only known once it has been applied: a variant that
    fails the structure check raises `UnsupportedSystem` after the replay, before any launch, and
    the optic is `reset()` to its nominal state first (the samplers have been drawn from).  The
    reference's own loop serves all of those.  After a successful call the optic is left as the
    last iteration left it, as `MonteCarlo.run` leaves it."""
    import torch

    optic = tolerancing.optic
    ops = _operand_cells(tolerancing)
    wavelengths = sorted({w for _hx, _hy, w, _n, _d in ops})
    pack_optic(optic, wavelengths)           # strict: UnsupportedSystem before anything moves
    names = [f"{i}: {op}" for i, op in enumerate(tolerancing.operands)]
    K = int(num_iterations)
    rows = [dict() for _ in range(K)]

    def mutate(_optic, k):    # MonteCarlo.run's own order
        tolerancing.reset()
        for p in tolerancing.perturbations:
            p.apply()
        for p in tolerancing.perturbations:
            rows[k][str(p.variable)] = float(p.value)

    tables = pack_ensemble(optic, mutate, K, wavelengths, restore=lambda _o: None)
    if K == 0:
        return rows
    try:
        check_structure(tables)
    except (StructureMismatch, UnsupportedStructure) as exc:
        tolerancing.reset()      # nothing is launched and the optic is the nominal one again
        raise UnsupportedSystem(f"monte_carlo_spots: {exc}") from exc
    dtype = torch.float64 if dtype is None else dtype
    values = np.zeros((K, len(ops)))
    groups: dict = {}
    for j, (_hx, _hy, _w, n, dist) in enumerate(ops):
        groups.setdefault((n, dist), []).append(j)
    if K < min_ensemble:
        _loop(tables, ops, groups, values, device, dtype)
    else:
        ens = SystemEnsemble(tables, device, dtype)
        try:
            _ensemble(ens, tables, ops, groups, values)
        finally:
            ens.close()
    for k in range(K):
        rows[k].update({name: float(values[k, j]) for j, name in enumerate(names)})
    return rows


def _cells_of(tables, ops, members, K):
    """(K, len(members)) cells: variant k, the operand's field and wavelength row."""
    cells = np.concatenate(
        [cell_grid(K, [ops[j][:2]], [tables[0].wavelength_index(ops[j][2])]).reshape(K, 1)
         for j in members], axis=1)
    return cells


def _finish(mom, hits, n, out):
    """Operand values of (cells, 8) moments / (cells, 3, n) hits into `out` (cells,)."""
    full = mom[:, 0] == n
    out[full] = rms_about_centroid(mom[full])
    for c in np.nonzero(~full)[0]:
        out[c] = operand_from_hits(hits[c, 0], hits[c, 1])


def _ensemble(ens, tables, ops, groups, values):
    import torch
    K = len(tables)
    zero = torch.zeros(1, dtype=ens.dtype, device=ens.device)
    for (n_rays, dist), members in groups.items():
        cells = _cells_of(tables, ops, members, K)
        # every cell about its OWN chief-ray hit: the sums then hold the spot, not the image height
        _m, chief = ens.trace_spot(zero, zero, cells, hits=True)
        c = chief[:, :2, 0].double().cpu().numpy().reshape(K, len(members), 2)
        cells["cx"], cells["cy"] = c[..., 0], c[..., 1]
        x, y = pupil_points(dist, n_rays)
        px = torch.from_numpy(x).to(device=ens.device, dtype=ens.dtype)
        py = torch.from_numpy(y).to(device=ens.device, dtype=ens.dtype)
        n = int(px.numel())
        # the moments alone first: in a tolerancing run few cells lose a ray, and only those are
        # traced once more with their hit planes
        mom = ens.trace_spot(px, py, cells)[0].cpu().numpy()
        out = np.zeros(K * len(members))
        lost = np.nonzero(mom[:, 0] != n)[0]
        hits = None
        if lost.size:
            _m, hb = ens.trace_spot(px, py, cells.reshape(-1)[lost], hits=True)
            hits = np.full((mom.shape[0], 3, n), np.nan)
            hits[lost] = hb[..., :n].double().cpu().numpy()
        _finish(mom, hits, n, out)
        values[:, members] = out.reshape(K, len(members))


def _loop(tables, ops, groups, values, device, dtype):
    """The same values variant by variant: one `HipSystem`, re-written in place per variant."""
    import torch

    from .engine import HipSystem
    hs = HipSystem(tables[0], device)
    try:
        for k, t in enumerate(tables):
            if k and not hs.update(t):
                hs.close()
                hs = HipSystem(t, device)
            for (n_rays, dist), members in groups.items():
                x, y = pupil_points(dist, n_rays)
                px = torch.from_numpy(x).to(device=hs.device, dtype=dtype)
                py = torch.from_numpy(y).to(device=hs.device, dtype=dtype)
                n = int(px.numel())
                zero = torch.zeros(1, dtype=dtype, device=hs.device)
                cells = [(ops[j][0], ops[j][1], 1.0, 1.0, 0.0, 0.0,
                          t.wavelength_index(ops[j][2])) for j in members]
                _m, chief = hs.trace_spot_batch(zero, zero, cells, hits=True)
                c = chief[:, :2, 0].double().cpu().numpy()
                cells = [cell[:4] + (float(c[i, 0]), float(c[i, 1])) + cell[6:]
                         for i, cell in enumerate(cells)]
                mom, hb = hs.trace_spot_batch(px, py, cells, hits=True)
                mom = mom.cpu().numpy()
                hits = hb[..., :n].double().cpu().numpy() if (mom[:, 0] != n).any() else None
                out = np.zeros(len(members))
                _finish(mom, hits, n, out)
                values[k, members] = out
    finally:
        hs.close()


# ------------------------------------------------------------------ wavefront operands
# Below this many iterations `monte_carlo` evaluates its `OPD_difference` operands variant by
# variant (`HipSystem.update` + `wavefront_reference` + `trace_opd`) instead of through the
# ensemble.  Measured on the MI355X (profiles/ensemble_opd.txt, tools/gpu_ensemble_opd.py, 3
# fields, 91 and 469 rays): the ensemble CALL is 100-108 x ahead of the loop at K = 64 (0.14-0.15
# against 15 ms) and 1330-1720 x at K = 4096 (0.50-0.65 against 858-871 ms); BUILDING the ensemble,
# once, is 8.9 ms at K = 64, 10.8 at 128, 12.8 at 256, 28 at 1024, 98 at 4096.  Build + call
# against the loop: 9.1 against 15 ms at K = 64, 11 against 30 at 128, 13 against 57 at 256, 28
# against 211-219 at 1024, 98 against 858-871 at 4096 -- ahead at every measured size, so the
# constant is the smallest size measured (the loop costs 0.23 ms per variant and the build starts
# at ~7 ms: the crossover lies below it, unmeasured).  The spot operands of the same problem keep
# ENSEMBLE_MIN_VARIANTS, unless the ensemble is built for the wavefronts anyway.
OPD_ENSEMBLE_MIN_VARIANTS = 64

_SPOT, _OPD = "rms_spot_size", "OPD_difference"


def _problem(tolerancing):
    """[(kind, Hx, Hy, wavelength, num_rays, distribution)] of the problem's operands, or
    UnsupportedSystem -- before anything is perturbed."""
    optic = tolerancing.optic
    last = len(optic.surfaces.surfaces) - 1
    if getattr(tolerancing.compensator, "has_variables", False):
        raise UnsupportedSystem("monte_carlo: compensators are not traced inside the launch")
    if not tolerancing.operands:
        raise ValueError("No operands found in the tolerancing system.")    # MonteCarlo._validate
    if not tolerancing.perturbations:
        raise ValueError("No perturbations found in the tolerancing system.")
    ops = []
    for i, op in enumerate(tolerancing.operands):
        if op.operand_type not in (_SPOT, _OPD):
            raise UnsupportedSystem(f"monte_carlo: operand {i} is {op.operand_type!r}, not "
                                    f"{_SPOT!r} or {_OPD!r}")
        d = dict(op.input_data)
        if d.get("optic") is not optic:
            raise UnsupportedSystem(f"monte_carlo: operand {i} reads another optic")
        if isinstance(d.get("wavelength"), str):
            raise UnsupportedSystem(f"monte_carlo: operand {i} has wavelength="
                                    f"{d['wavelength']!r} (one wavelength per operand)")
        if op.operand_type == _SPOT:
            s = int(d["surface_number"])
            if s not in (-1, last):
                raise UnsupportedSystem(f"monte_carlo: operand {i} reads surface {s}, not the "
                                        f"image surface")
            dist = str(d.get("distribution", "hexapolar"))
        else:
            dist = d.get("distribution", "gaussian_quad")
            if not isinstance(dist, str):
                raise UnsupportedSystem(f"monte_carlo: operand {i} carries a distribution object "
                                        f"(name one)")
        ops.append((op.operand_type, float(d["Hx"]), float(d["Hy"]), float(d["wavelength"]),
                    int(d["num_rays"]), dist))
    return ops


def operand_from_opd(opd, weights=1.0) -> float:
    """`RayOperand.OPD_difference` on an OPD map in waves (optimization/operand/ray.py:387-389):
    mean(|(opd - mean opd) * weights|) over ALL rays, clipped rays included, NaN included."""
    opd = np.asarray(opd, dtype=np.float64)
    return float(np.mean(np.abs((opd - np.mean(opd)) * weights)))


def opd_operand_points(distribution: str, num_rays: int, on_axis: bool):
    """(px, py, weights) an `OPD_difference` operand traces: for "gaussian_quad" the points and
    weights of the reference's own `GaussianQuadrature` (symmetric on axis: `num_rays` points,
    else 3 x `num_rays`; ray.py:369-377), for any other name that sampler's points, weights 1."""
    if distribution != "gaussian_quad":
        x, y = pupil_points(distribution, num_rays)
        return x, y, 1.0
    import optiland.backend as be
    from optiland.distribution import GaussianQuadrature
    d = GaussianQuadrature(is_symmetric=on_axis)
    w = d.get_weights(num_rays)
    d.generate_points(num_rings=num_rays)

    def host(v):
        return np.asarray(be.to_numpy(v), dtype=np.float64).reshape(-1)

    return host(d.x), host(d.y), host(w) if on_axis else np.repeat(host(w), 3)


def monte_carlo(tolerancing, num_iterations: int, device=None, dtype=None,
                min_ensemble: int | None = None) -> list:
    """`MonteCarlo(tolerancing).run(num_iterations)` for problems whose operands are
    `rms_spot_size` and `OPD_difference` at one wavelength each and which have no compensators.
    The replay, the rows returned and the refusals are `monte_carlo_spots`'s; the spot operands
    are evaluated as there.  The `OPD_difference` operands are grouped by (num_rays, distribution,
    Hx == Hy == 0) -- one set of pupil points and weights per group -- and every cell of a group
    goes in ONE `SystemEnsemble.trace_opd` call with its OPD planes; the value is formed on the
    host from the cell's plane exactly as the operand forms it (an unmasked mean).  With fewer
    than `min_ensemble` iterations every operand is evaluated variant by variant instead
    (default: OPD_ENSEMBLE_MIN_VARIANTS for the wavefront operands, ENSEMBLE_MIN_VARIANTS for the
    spot operands -- which ride an ensemble that is built for the wavefronts anyway).
    `dtype` is the spot operands'; wavefronts are fp64."""
    import torch

    optic = tolerancing.optic
    ops = _problem(tolerancing)
    wavelengths = sorted({op[3] for op in ops})
    nominal = pack_optic(optic, wavelengths)   # strict: UnsupportedSystem before anything moves
    opd_members = [j for j, op in enumerate(ops) if op[0] == _OPD]
    if opd_members:
        if "pupil_z" not in nominal.raygen or "n_image" not in nominal.raygen:
            raise UnsupportedSystem("monte_carlo: this optic packs no exit-pupil data")
        if any(float(f[2]) != 0.0 or float(f[3]) != 0.0 for f in nominal.fields):
            raise UnsupportedSystem("monte_carlo: vignetted fields are not served for "
                                    f"{_OPD!r} operands")
    names = [f"{i}: {op}" for i, op in enumerate(tolerancing.operands)]
    K = int(num_iterations)
    rows = [dict() for _ in range(K)]

    def mutate(_optic, k):    # MonteCarlo.run's own order
        tolerancing.reset()
        for p in tolerancing.perturbations:
            p.apply()
        for p in tolerancing.perturbations:
            rows[k][str(p.variable)] = float(p.value)

    tables = pack_ensemble(optic, mutate, K, wavelengths, restore=lambda _o: None)
    if K == 0:
        return rows
    try:
        check_structure(tables)
    except (StructureMismatch, UnsupportedStructure) as exc:
        tolerancing.reset()      # nothing is launched and the optic is the nominal one again
        raise UnsupportedSystem(f"monte_carlo: {exc}") from exc
    dtype = torch.float64 if dtype is None else dtype
    values = np.zeros((K, len(ops)))
    # the spot operands: `monte_carlo_spots`'s tuples and groups, in a block of their own
    spot_members = [j for j, op in enumerate(ops) if op[0] == _SPOT]
    spot_ops = [ops[j][1:] for j in spot_members]
    spot_groups: dict = {}
    for i, (_hx, _hy, _w, n, dist) in enumerate(spot_ops):
        spot_groups.setdefault((n, dist), []).append(i)
    spot_values = np.zeros((K, len(spot_ops)))
    opd_groups: dict = {}
    for j in opd_members:
        _kind, hx, hy, _w, n, dist = ops[j]
        opd_groups.setdefault((n, dist, hx == hy == 0), []).append(j)
    opd_ens = bool(opd_members) and \
        K >= (OPD_ENSEMBLE_MIN_VARIANTS if min_ensemble is None else min_ensemble)
    spot_ens = bool(spot_ops) and \
        (opd_ens or K >= (ENSEMBLE_MIN_VARIANTS if min_ensemble is None else min_ensemble))
    if spot_ops and not spot_ens:
        _loop(tables, spot_ops, spot_groups, spot_values, device, dtype)
    if opd_members and not opd_ens:
        _opd_loop(tables, ops, opd_groups, values, device)
    if spot_ens or opd_ens:
        # ONE ensemble for both kinds of operand (it holds the tables of both precisions; its
        # dtype is that of the pupil planes it is handed, and wavefronts are fp64)
        ens = SystemEnsemble(tables, device, dtype)
        try:
            if spot_ens:
                _ensemble(ens, tables, spot_ops, spot_groups, spot_values)
            if opd_ens:
                ens.dtype = torch.float64
                _opd_ensemble(ens, tables, ops, opd_groups, values)
        finally:
            ens.close()
    values[:, spot_members] = spot_values
    for k in range(K):
        rows[k].update({name: float(values[k, j]) for j, name in enumerate(names)})
    return rows


def _opd_ensemble(ens, tables, ops, groups, values):
    import torch

    from .ensemble import opd_cell_grid
    K = len(tables)
    for (n_rays, dist, on_axis), members in groups.items():
        x, y, weights = opd_operand_points(dist, n_rays, on_axis)
        px = torch.from_numpy(x).to(device=ens.device, dtype=torch.float64)
        py = torch.from_numpy(y).to(device=ens.device, dtype=torch.float64)
        n = int(px.numel())
        cells = np.concatenate(
            [opd_cell_grid(tables, [ops[j][1:3]],
                           [tables[0].wavelength_index(ops[j][3])]).reshape(K, 1)
             for j in members], axis=1)
        _m, _r, planes = ens.trace_opd(px, py, cells, planes=True)
        opd = planes[:, 0, :n].cpu().numpy().reshape(K, len(members), n)
        for i, j in enumerate(members):
            values[:, j] = [operand_from_opd(opd[k, i], weights) for k in range(K)]


def _opd_loop(tables, ops, groups, values, device):
    """The same values variant by variant: one `HipSystem`, re-written in place per variant, and
    per operand the two single launches."""
    import torch

    from .analysis_seams import _launch_plane_tilt
    from .engine import HipSystem
    hs = HipSystem(tables[0], device)
    points = {key: opd_operand_points(key[1], key[0], key[2]) for key in groups}
    try:
        for k, t in enumerate(tables):
            if k and not hs.update(t):
                hs.close()
                hs = HipSystem(t, device)
            rg = t.raygen
            for key, members in groups.items():
                x, y, weights = points[key]
                px = torch.from_numpy(x).to(device=hs.device, dtype=torch.float64)
                py = torch.from_numpy(y).to(device=hs.device, dtype=torch.float64)
                for j in members:
                    _kind, hx, hy, w, _n, _dist = ops[j]
                    wl = t.wavelength_index(w)
                    ux, uy = _launch_plane_tilt(rg, hx, hy)
                    params = dict(n_image=rg["n_image"], ux=ux, uy=uy, half_epd=rg["EPD"] / 2.0,
                                  wavelength_um=float(t.wavelengths[wl]),
                                  last_thickness=float(t.last_thickness))
                    ref, _chief = hs.wavefront_reference(params, wl, field=(hx, hy),
                                                         pupil_z=rg["pupil_z"])
                    opd, _i, _p, _m = hs.trace_opd(None, px, py, wl, field=(hx, hy),
                                                   want_pupil=False, reference=ref,
                                                   zero_status=False)
                    values[k, j] = operand_from_opd(opd.cpu().numpy(), weights)
    finally:
        hs.close()
