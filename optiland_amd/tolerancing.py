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
