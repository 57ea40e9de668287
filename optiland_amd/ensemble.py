"""K variants of one optic on the device, traced and reduced in ONE launch (`ol_ensemble_*`,
`ol_trace_spot_ensemble`).

What Monte Carlo tolerancing, a sensitivity table, a finite-difference Jacobian or a population
optimiser do is trace a few hundred rays through thousands of variants of one lens; through
`HipSystem` that is one table upload, one launch and one status read-back per variant, all of it
overhead.  `SystemEnsemble` keeps the variants' tables stacked on the device (the variants share
their STRUCTURE and differ in values); `trace_spot` traces any grid of (variant, field,
wavelength) cells over one set of pupil points in one launch and reads the status word back once.
`EnsembleSpot` is the stand-alone analysis on top: centroid, RMS and geometric spot radius as
(K, F, W) arrays, with `analysis.SpotDiagram`'s definitions.

`trace_opd` (`ol_trace_opd_ensemble`) does the same for wavefronts: every cell's chief-ray
reference, OPD map and the twelve moments of `ol_trace_opd` in two launches for all cells;
`EnsembleWavefront` is the analysis on top (RMS, mean and reference radius as (K, F, W) arrays,
with `wavefront.OPD`'s definitions).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import system as S
from .system import SystemTable

# What the variants of an ensemble must share, per surface: everything that selects code or
# layout (csrc/ensemble_rules.h states the same rules, with the same texts, for the library).
# SURF_ROTATED says what rot[] holds -- a tilt tolerance sets it on one variant only -- and is a
# run-time branch on the variant's own row.
STRUCTURE_FIELDS = ("geom_kind", "interaction", "aperture_kind", "coating_kind", "flags",
                    "n_coeff", "coeff_offset", "poly_cols")
_FLAG_MASK = 0xFFFFFFFF & ~S.SURF_ROTATED
_SHARE = "(the variants of an ensemble share their structure)"


class StructureMismatch(ValueError):
    """A variant differs from variant 0 in something that selects code or layout."""


def _structure_columns(surfaces) -> np.ndarray:
    """(surfaces, len(STRUCTURE_FIELDS)) int64: what is compared, in the order it is compared."""
    cols = [surfaces[n].astype(np.int64) & _FLAG_MASK if n == "flags"
            else surfaces[n].astype(np.int64) for n in STRUCTURE_FIELDS]
    return np.stack(cols, axis=1)


def _raygen_structure(rg: dict):
    return (("object_infinite", int(bool(rg.get("object_infinite", 0)))),
            ("field_kind", int(rg.get("field_kind", 0))),
            ("apod_kind", int(rg.get("apod_kind", 0))),
            ("telecentric", int(float(rg.get("tele_dz", 0.0)) > 0.0)))


def check_structure(tables, first: int = 0, reference: SystemTable | None = None,
                    who: str = "ol_ensemble_create") -> None:
    """Every table of `tables` (variants `first`, `first + 1`, ...) against `reference` (default:
    `tables[0]`, variant 0).  Raises `StructureMismatch` naming the variant, the surface and the
    field, and `UnsupportedStructure` for what no ensemble launch serves (one-launch kinds,
    reference-rule Newton surfaces)."""
    ref = tables[0] if reference is None else reference
    if not ref.raygen:
        raise ValueError(f"{who}: variant 0 carries no ray-generation scalars")
    for i, kind in sorted(ref.single_rows.items()):
        raise UnsupportedStructure(
            f"{who}: surface {i} is {kind.noun}: an ensemble launch walks the whole system in one "
            f"kernel")
    if ref.reference_newton_surfaces():
        raise UnsupportedStructure(
            f"{who}: the system carries OL_SURF_REFERENCE_NEWTON surfaces (reference stop rule): "
            f"their iteration count is a property of the batch")
    rs = ref.surfaces
    for j, t in enumerate(tables):
        k = first + j
        if t is ref:
            continue
        if t.num_surfaces != ref.num_surfaces:
            raise StructureMismatch(f"{who}: variant {k}: {t.num_surfaces} surfaces differ from "
                                    f"variant 0's {ref.num_surfaces} {_SHARE}")
        if t.optics.shape[1] != ref.optics.shape[1]:
            raise StructureMismatch(f"{who}: variant {k}: n_wl {t.optics.shape[1]} differs from "
                                    f"variant 0's {ref.optics.shape[1]} {_SHARE}")
        want, got = _structure_columns(rs), _structure_columns(t.surfaces)
        bad = np.argwhere(want != got)   # row-major: the first surface, on it the first field
        if bad.size:
            s, j = (int(v) for v in bad[0])
            raise StructureMismatch(f"{who}: variant {k}, surface {s}: {STRUCTURE_FIELDS[j]} "
                                    f"{int(got[s, j])} differs from variant 0's {int(want[s, j])} "
                                    f"{_SHARE}")
        if t.coeffs.size != ref.coeffs.size:
            raise StructureMismatch(f"{who}: variant {k}: coefficient buffer of {t.coeffs.size} "
                                    f"values differs from variant 0's {ref.coeffs.size} {_SHARE}")
        if not t.raygen:
            raise ValueError(f"{who}: variant {k} carries no ray-generation scalars")
        for (name, want), (_n, got) in zip(_raygen_structure(ref.raygen),
                                           _raygen_structure(t.raygen)):
            if want != got:
                raise StructureMismatch(f"{who}: variant {k}: raygen {name} {got} differs from "
                                        f"variant 0's {want} {_SHARE}")
        if (t.polarization is None) != (ref.polarization is None):
            raise StructureMismatch(f"{who}: variant {k}: polarization "
                                    f"{'set' if t.polarization is not None else 'ignored'} differs "
                                    f"from variant 0's {_SHARE}")


class UnsupportedStructure(ValueError):
    """The optic holds something no ensemble launch serves (a one-launch kind, a reference-rule
    Newton surface)."""


def cell_grid(n_variants: int, fields, wavelength_indices, centers=None, vig=None) -> np.ndarray:
    """The (K, F, W) grid of cells as a structured array (`_capi.EnsembleCell` layout), variant
    slowest, wavelength fastest: cell (k, f, w) is record (k * F + f) * W + w.  `fields`: F pairs
    (Hx, Hy); `centers`: (F, 2) or (K, F, 2) or (K, F, W, 2) centres of the moments (default 0);
    `vig`: F pairs (1 - vx, 1 - vy) (default unvignetted)."""
    f = np.asarray(fields, dtype=np.float64).reshape(-1, 2)
    wl = np.asarray(wavelength_indices, dtype=np.int32).reshape(-1)
    K, F, W = int(n_variants), f.shape[0], wl.shape[0]
    cells = np.zeros((K, F, W), dtype=CELL_DTYPE)
    cells["variant"] = np.arange(K, dtype=np.int32)[:, None, None]
    cells["wavelength_index"] = wl[None, None, :]
    cells["hx"] = f[None, :, 0, None]
    cells["hy"] = f[None, :, 1, None]
    v = np.ones((F, 2)) if vig is None else np.asarray(vig, dtype=np.float64).reshape(F, 2)
    cells["vx"] = v[None, :, 0, None]
    cells["vy"] = v[None, :, 1, None]
    if centers is not None:
        c = np.asarray(centers, dtype=np.float64)
        if c.shape == (F, 2):
            c = c[None, :, None, :]
        elif c.shape == (K, F, 2):
            c = c[:, :, None, :]
        elif c.shape != (K, F, W, 2):
            raise ValueError("centers must be (F, 2), (K, F, 2) or (K, F, W, 2)")
        cells["cx"] = np.broadcast_to(c[..., 0], (K, F, W))
        cells["cy"] = np.broadcast_to(c[..., 1], (K, F, W))
    return cells


CELL_DTYPE = np.dtype([("variant", np.int32), ("wavelength_index", np.int32), ("hx", np.float64),
                       ("hy", np.float64), ("vx", np.float64), ("vy", np.float64),
                       ("cx", np.float64), ("cy", np.float64)], align=True)
assert CELL_DTYPE.itemsize == C.sizeof(_capi.EnsembleCell)

OPD_CELL_DTYPE = np.dtype([("variant", np.int32), ("wavelength_index", np.int32),
                           ("hx", np.float64), ("hy", np.float64), ("vx", np.float64),
                           ("vy", np.float64), ("n_image", np.float64), ("pupil_z", np.float64),
                           ("wavelength_um", np.float64), ("last_thickness", np.float64),
                           ("planar", np.int32), ("reserved_", np.int32)], align=True)
assert OPD_CELL_DTYPE.itemsize == C.sizeof(_capi.EnsembleOpdCell)


def opd_cell_grid(tables, fields, wavelength_indices, vig=None, planar: bool = False) -> np.ndarray:
    """The (K, F, W) grid of wavefront cells (`_capi.EnsembleOpdCell` layout), ordered like
    `cell_grid`.  What the ensemble does not store is taken from EACH variant's own table: the
    image-space index and the exit-pupil position of its `raygen`, its last thickness; the
    wavelength in microns is the table's at that row.  `planar`: afocal, every cell against the
    plane through its chief ray's hit."""
    tables = list(tables)
    f = np.asarray(fields, dtype=np.float64).reshape(-1, 2)
    wl = np.asarray(wavelength_indices, dtype=np.int32).reshape(-1)
    K, F, W = len(tables), f.shape[0], wl.shape[0]
    cells = np.zeros((K, F, W), dtype=OPD_CELL_DTYPE)
    cells["variant"] = np.arange(K, dtype=np.int32)[:, None, None]
    cells["wavelength_index"] = wl[None, None, :]
    cells["hx"] = f[None, :, 0, None]
    cells["hy"] = f[None, :, 1, None]
    v = np.ones((F, 2)) if vig is None else np.asarray(vig, dtype=np.float64).reshape(F, 2)
    cells["vx"] = v[None, :, 0, None]
    cells["vy"] = v[None, :, 1, None]
    cells["planar"] = 1 if planar else 0
    for k, t in enumerate(tables):
        rg = t.raygen
        if "pupil_z" not in rg or "n_image" not in rg:
            raise ValueError("this SystemTable carries no exit-pupil data")
        cells["n_image"][k] = float(rg["n_image"])
        cells["pupil_z"][k] = float(rg["pupil_z"])
        cells["last_thickness"][k] = float(t.last_thickness)
        cells["wavelength_um"][k] = np.asarray(t.wavelengths, dtype=np.float64)[wl][None, :]
    return cells


def opd_statistics(moments) -> tuple:
    """(RMS, mean) of the OPD in waves over the rays that arrive, from (..., 12) moments, with
    `wavefront.OPD`'s definitions: RMS = sqrt(sum o^2 / count) (opd.py:145-159), mean =
    sum o / count.  A cell without a surviving ray gives NaN."""
    m = np.asarray(moments, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(m[..., 11] / m[..., 9]), m[..., 10] / m[..., 9]


def radii_from_moments(moments) -> tuple:
    """(centroid offset x, centroid offset y, RMS radius, geometric radius) from (..., 8) moments
    about the cells' centres, in fp64, with `analysis.SpotDiagram`'s definitions: centroid =
    centre + sum d / count, RMS = sqrt(max((sum dx^2 + sum dy^2) / count, 0)), geometric =
    sqrt(max r^2).  A cell without a surviving ray (count 0) gives NaN centroid and RMS."""
    m = np.asarray(moments, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = m[..., 0]
        dx, dy = m[..., 1] / n, m[..., 2] / n
        rms = np.sqrt(np.maximum((m[..., 3] + m[..., 4]) / n, 0.0))
    return dx, dy, rms, np.sqrt(m[..., 6])


def rms_about_centroid(moments) -> np.ndarray:
    """RMS radius about each cell's OWN centroid, from the sums about the centre:
    sqrt(max((sum dx^2 + sum dy^2) / n - (sum dx / n)^2 - (sum dy / n)^2, 0))."""
    m = np.asarray(moments, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = m[..., 0]
        v = (m[..., 3] + m[..., 4]) / n - (m[..., 1] / n) ** 2 - (m[..., 2] / n) ** 2
    return np.sqrt(np.maximum(v, 0.0))


class SystemEnsemble:
    """K packed variants of one optic resident on one GPU (wraps `ol_ensemble`)."""

    def __init__(self, tables, device=None, dtype=None):
        import torch

        from .engine import _require_gpu
        tables = list(tables)
        if not tables:
            raise ValueError("SystemEnsemble: no variants")
        check_structure(tables)
        self.lib = _capi.load()
        if not _capi.has_ensemble(self.lib):
            raise _capi.HipExtensionError("this library has no ol_ensemble_* entries: rebuild")
        self.device = _require_gpu(device)
        self.dtype = torch.float64 if dtype is None else dtype
        if self.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"unsupported ray dtype {self.dtype}")
        self.tables = tables
        recs, keep = self._records(tables)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.ol_ensemble_create(recs, len(tables), tables[0].num_surfaces,
                                             tables[0].optics.shape[1], C.byref(handle))
        del keep
        _capi.check(rc, "ol_ensemble_create", self.lib)
        self._handle = handle
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)

    @staticmethod
    def _raygen_params(rg: dict):
        return _capi.RaygenParams(int(rg["object_infinite"]), int(rg.get("field_kind", 0)),
                                  rg["EPL"], rg["EPD"],
                                  float(rg.get("field_scale", rg["max_field"])), rg["offset"],
                                  rg["z_first"], float(rg.get("tele_dz", 0.0)),
                                  float(rg.get("apod_a", 0.0)), float(rg.get("apod_b", 0.0)),
                                  int(rg.get("apod_kind", 0)), 0)

    @classmethod
    def _records(cls, tables):
        """(`ol_ensemble_variant` array, keep-alive list) of packed tables."""
        keep, recs = [], (_capi.EnsembleVariant * len(tables))()
        for i, t in enumerate(tables):
            surf = np.ascontiguousarray(t.surfaces)
            optics = np.ascontiguousarray(t.optics)
            coeffs = np.ascontiguousarray(t.coeffs, dtype=np.float64)
            rg = cls._raygen_params(t.raygen)
            keep += [surf, optics, coeffs, rg]
            recs[i] = _capi.EnsembleVariant(surf.ctypes.data,
                                            coeffs.ctypes.data if coeffs.size else None,
                                            optics.ctypes.data, C.addressof(rg), coeffs.size, 0)
        return recs, keep

    def __len__(self) -> int:
        return len(self.tables)

    @property
    def size(self) -> int:
        """`ol_ensemble_size`."""
        return int(self.lib.ol_ensemble_size(self._handle)) if self._handle else 0

    def _stream(self) -> int:
        from .engine import _stream_ptr
        return _stream_ptr(self.device)

    def update(self, k: int, table) -> None:
        """`ol_ensemble_update`: rewrite variant `k` (or, with a list of tables, variants
        k, k + 1, ...) in place -- no allocation, the copies are queued on the current stream
        behind every launch that still reads the old rows."""
        import torch
        new = list(table) if isinstance(table, (list, tuple)) else [table]
        k = int(k)
        if k < 0 or k + len(new) > len(self.tables):
            raise IndexError(f"variants [{k}, {k + len(new)}) outside [0, {len(self.tables)})")
        check_structure(new, first=k, reference=self.tables[0], who="ol_ensemble_update")
        recs, keep = self._records(new)
        with torch.cuda.device(self.device):
            rc = self.lib.ol_ensemble_update(self._handle, k, len(new), recs, self._stream())
        del keep
        _capi.check(rc, "ol_ensemble_update", self.lib)
        self.tables[k: k + len(new)] = new

    def trace_spot(self, px, py, cells, hits: bool = False, out=None, check_status: bool = True,
                   flags: int = 0):
        """`ol_trace_spot_ensemble`: every cell of `cells` -- a `cell_grid` array (any shape), or
        a device uint8 tensor already holding such records -- traces the pupil planes `px`, `py`
        through its variant, ONE launch.  Returns (moments, hits): moments a (cells, 8) float64
        device tensor (per cell {count, sum dx, sum dy, sum dx^2, sum dy^2, sum i, max r^2, -};
        `out`, if given, is accumulated into), hits None or a (cells, 3, stride) block of the
        image-plane x, y, intensity (use `[..., :n]`).  The status word is read back once."""
        import torch
        if getattr(self, "_handle", None) is None:
            raise _capi.HipExtensionError("trace_spot: this ensemble is closed")
        n, dtype = int(px.numel()), px.dtype
        if dtype != self.dtype or py.dtype != dtype or py.numel() != n \
                or px.device != self.device or py.device != self.device:
            raise ValueError("trace_spot: px, py must be planes of the ensemble's dtype on its "
                             "device, equally long")
        if isinstance(cells, torch.Tensor):
            if cells.dtype != torch.uint8 or cells.device != self.device \
                    or cells.numel() % CELL_DTYPE.itemsize or not cells.is_contiguous():
                raise ValueError("trace_spot: device cells must be a contiguous uint8 tensor of "
                                 "whole ol_ensemble_cell records on the ensemble's device")
            cells_dev = cells
        else:
            host = np.ascontiguousarray(np.asarray(cells, dtype=CELL_DTYPE).reshape(-1))
            cells_dev = torch.from_numpy(host.view(np.uint8)).to(self.device)
        k = cells_dev.numel() // CELL_DTYPE.itemsize
        if out is None:
            out = torch.zeros((k, 8), dtype=torch.float64, device=self.device)
        elif out.shape != (k, 8) or out.dtype != torch.float64 or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError("out must be a contiguous (cells, 8) float64 tensor on the device")
        hb, stride = None, 0
        if hits:
            b = px.element_size()
            stride = (n + 16 // b - 1) // (16 // b) * (16 // b)   # planes stay 16-byte aligned
            hb = torch.empty((k, 3, max(stride, 1)), dtype=dtype, device=self.device)
        if n == 0 or k == 0:
            return out, hb
        px, py = px.contiguous(), py.contiguous()
        inp = _capi.RaygenInputs(None, None, px.data_ptr(), py.data_ptr(), None, None, 0.0, 0.0,
                                 1.0, 1.0, int(flags), 0)
        if check_status:
            self._status.zero_()
        with torch.cuda.device(self.device):
            rc = self.lib.ol_trace_spot_ensemble(
                self._handle, _capi.F32 if dtype == torch.float32 else _capi.F64, n, C.byref(inp),
                k, cells_dev.data_ptr(), hb.data_ptr() if hb is not None else None, stride,
                out.data_ptr(), self._status.data_ptr(), self._stream())
        _capi.check(rc, "ol_trace_spot_ensemble", self.lib)
        if check_status:
            self.raise_for_status(int(self._status.item()))
        return out, hb

    def trace_opd(self, px, py, cells, planes=False, pupil: bool = False,
                  check_status: bool = True, out=None, refs=None, stride: int | None = None,
                  flags: int = 0):
        """`ol_trace_opd_ensemble`: every cell of `cells` -- an `opd_cell_grid` array (any shape),
        or a device uint8 tensor already holding such records -- gets its chief-ray reference
        and the OPD of the pupil planes `px`, `py` against it: TWO launches for all cells, no
        read-back between them.  Returns (moments, refs, planes): moments a (cells, 12) float64
        device tensor (the twelve of `ol_trace_opd`; `out`, if given, is accumulated into), refs
        (cells, 16) (`[:, 0:3]` centre, `[:, 3]` radius; `refs`, if given, is written), planes
        None or a (cells, P, stride) block -- P = 2: OPD in waves and intensity, P = 5 with
        `pupil`: + the pupil point (use `[..., :n]`); a tensor passed as `planes` is written in
        place.  fp64 ensembles only.  The status word is read back once."""
        import torch
        if getattr(self, "_handle", None) is None:
            raise _capi.HipExtensionError("trace_opd: this ensemble is closed")
        if not _capi.has_ensemble_opd(self.lib):
            raise _capi.HipExtensionError("this library has no ol_trace_opd_ensemble: rebuild")
        if self.dtype != torch.float64:
            raise ValueError("trace_opd: wavefront work is fp64 only (an fp64 ensemble)")
        n = int(px.numel())
        if px.dtype != torch.float64 or py.dtype != torch.float64 or py.numel() != n \
                or px.device != self.device or py.device != self.device:
            raise ValueError("trace_opd: px, py must be float64 planes on the ensemble's device, "
                             "equally long")
        size = OPD_CELL_DTYPE.itemsize
        if isinstance(cells, torch.Tensor):
            if cells.dtype != torch.uint8 or cells.device != self.device \
                    or cells.numel() % size or not cells.is_contiguous():
                raise ValueError("trace_opd: device cells must be a contiguous uint8 tensor of "
                                 "whole ol_ensemble_opd_cell records on the ensemble's device")
            cells_dev = cells
        else:
            host = np.ascontiguousarray(np.asarray(cells, dtype=OPD_CELL_DTYPE).reshape(-1))
            cells_dev = torch.from_numpy(host.view(np.uint8)).to(self.device)
        k = cells_dev.numel() // size
        nref, P = _capi.WAVEFRONT_REFERENCE_DOUBLES, 5 if pupil else 2

        def block(t, shape, what, fresh):
            if t is None:
                return fresh(shape, dtype=torch.float64, device=self.device)
            if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous() \
                    or t.device != self.device:
                raise ValueError(f"{what} must be a contiguous {shape} float64 tensor on the "
                                 f"device")
            return t

        out = block(out, (k, _capi.OPD_MOMENTS), "out", torch.zeros)
        refs = block(refs, (k, nref), "refs", torch.zeros)
        pb = None
        if isinstance(planes, torch.Tensor):
            stride = int(planes.shape[-1]) if planes.dim() == 3 else -1
            pb = block(planes, (k, P, stride), "planes", torch.empty)
            if stride < n:
                raise ValueError(f"planes: stride {stride} < {n} rays")
        elif planes:
            stride = max(n if stride is None else int(stride), 1)
            if stride < n:
                raise ValueError(f"planes: stride {stride} < {n} rays")
            pb = torch.empty((k, P, stride), dtype=torch.float64, device=self.device)
        if n == 0 or k == 0:
            return out, refs, pb
        px, py = px.contiguous(), py.contiguous()
        inp = _capi.RaygenInputs(None, None, px.data_ptr(), py.data_ptr(), None, None, 0.0, 0.0,
                                 1.0, 1.0, int(flags) | (_capi.OPD_ENSEMBLE_PUPIL if pupil else 0),
                                 0)
        if check_status:
            self._status.zero_()
        with torch.cuda.device(self.device):
            rc = self.lib.ol_trace_opd_ensemble(
                self._handle, _capi.F64, n, C.byref(inp), k, cells_dev.data_ptr(),
                refs.data_ptr(), pb.data_ptr() if pb is not None else None,
                stride if pb is not None else 0, out.data_ptr(), self._status.data_ptr(),
                self._stream())
        _capi.check(rc, "ol_trace_opd_ensemble", self.lib)
        if check_status:
            self.raise_for_status(int(self._status.item()))
        return out, refs, pb

    @staticmethod
    def raise_for_status(status: int) -> None:
        if status & _capi.STATUS_ENSEMBLE_CELL:
            raise IndexError("ol_trace_spot_ensemble: a cell names a variant or a wavelength row "
                             "the ensemble does not hold")
        from .engine import HipSystem
        HipSystem.raise_for_status(status)

    def close(self):
        if getattr(self, "_handle", None):
            self.lib.ol_ensemble_destroy(self._handle)
            self._handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def pupil_points(distribution: str, num_rays: int):
    """(x, y) float64 pupil points of one of the reference's samplers."""
    from .distribution import create_distribution
    d = create_distribution(distribution)
    d.generate_points(num_rays)
    return np.asarray(d.x, dtype=np.float64), np.asarray(d.y, dtype=np.float64)


class EnsembleSpot:
    """Spot statistics of every variant of an ensemble: ONE launch for all K x F x W cells.

    `fields`: normalised (Hx, Hy) pairs, or "all" (the nominal table's field points);
    `wavelengths`: microns, or "all"; `num_rays`, `distribution`: as `SpotDiagram`'s `num_rings`
    and `distribution` (hexapolar: rings).  `centers`: (F, 2) global image coordinates the
    moments are taken about; default the NOMINAL variant's (variant 0) chief-ray hits at the
    reference wavelength -- one more one-ray launch."""

    def __init__(self, ensemble: SystemEnsemble, fields="all", wavelengths="all",
                 num_rays: int = 6, distribution: str = "hexapolar", centers=None):
        import torch
        self.ensemble = ensemble
        table = ensemble.tables[0]
        mf = table.raygen.get("max_field", 0.0) or 1.0
        if isinstance(fields, str) and fields == "all":
            fields = [(f[0] / mf, f[1] / mf) for f in table.fields]
        self.fields = [tuple(map(float, f[:2])) for f in fields]
        if isinstance(wavelengths, str) and wavelengths == "all":
            wavelengths = list(map(float, table.wavelengths))
        self.wavelengths = [float(w) for w in wavelengths]
        self.wl_index = [table.wavelength_index(w) for w in self.wavelengths]
        self.ref_index = table.reference_wavelength_index(self.wavelengths)
        K, F, W = len(ensemble), len(self.fields), len(self.wavelengths)
        dev, dt = ensemble.device, ensemble.dtype
        if centers is None:
            zero = torch.zeros(1, dtype=dt, device=dev)
            chief = cell_grid(1, self.fields, [self.wl_index[self.ref_index]])
            _m, hb = ensemble.trace_spot(zero, zero, chief, hits=True)
            centers = hb[:, :2, 0].double().cpu().numpy().reshape(F, 2)
        self.centers = np.asarray(centers, dtype=np.float64).reshape(F, 2)
        x, y = pupil_points(distribution, num_rays)
        px = torch.from_numpy(x).to(device=dev, dtype=dt)
        py = torch.from_numpy(y).to(device=dev, dtype=dt)
        self.num_points = int(px.numel())
        self.cells = cell_grid(K, self.fields, self.wl_index, centers=self.centers)
        mom, _ = ensemble.trace_spot(px, py, self.cells)
        self.moments = mom.cpu().numpy().reshape(K, F, W, 8)

    def centroid(self) -> np.ndarray:
        """(K, F, W, 2): centroid of every cell's surviving rays, global image coordinates."""
        dx, dy, _r, _g = radii_from_moments(self.moments)
        c = self.centers[None, :, None, :]
        return np.stack([c[..., 0] + dx, c[..., 1] + dy], axis=-1)

    def rms_spot_radius(self) -> np.ndarray:
        """(K, F, W): sqrt(mean((x - cx)^2 + (y - cy)^2)) about the centres."""
        return radii_from_moments(self.moments)[2]

    def rms_about_centroid(self) -> np.ndarray:
        """(K, F, W): RMS radius about each cell's own centroid (from the same sums)."""
        return rms_about_centroid(self.moments)

    def geometric_spot_radius(self) -> np.ndarray:
        """(K, F, W): max sqrt((x - cx)^2 + (y - cy)^2) about the centres."""
        return radii_from_moments(self.moments)[3]


class EnsembleWavefront:
    """OPD statistics of every variant of an ensemble against its own chief-ray reference: TWO
    launches for all K x F x W cells.

    `fields`, `wavelengths`: as `EnsembleSpot`; `num_rays`, `distribution`: as `wavefront.OPD`
    (hexapolar: rings).  `maps`: keep the per-ray planes -- `.opd` and `.intensity` are then
    (K, F, W, N) arrays (None otherwise).  `planar`: afocal, plane references.  `vig`: F pairs
    (1 - vx, 1 - vy) (default unvignetted)."""

    def __init__(self, ensemble: SystemEnsemble, fields="all", wavelengths="all",
                 num_rays: int = 6, distribution: str = "hexapolar", maps: bool = False,
                 planar: bool = False, vig=None):
        import torch
        self.ensemble = ensemble
        table = ensemble.tables[0]
        mf = table.raygen.get("max_field", 0.0) or 1.0
        if isinstance(fields, str) and fields == "all":
            fields = [(f[0] / mf, f[1] / mf) for f in table.fields]
        self.fields = [tuple(map(float, f[:2])) for f in fields]
        if isinstance(wavelengths, str) and wavelengths == "all":
            wavelengths = list(map(float, table.wavelengths))
        self.wavelengths = [float(w) for w in wavelengths]
        self.wl_index = [table.wavelength_index(w) for w in self.wavelengths]
        K, F, W = len(ensemble), len(self.fields), len(self.wavelengths)
        x, y = pupil_points(distribution, num_rays)
        px = torch.from_numpy(x).to(device=ensemble.device, dtype=torch.float64)
        py = torch.from_numpy(y).to(device=ensemble.device, dtype=torch.float64)
        self.num_points = n = int(px.numel())
        self.cells = opd_cell_grid(ensemble.tables, self.fields, self.wl_index, vig=vig,
                                   planar=planar)
        mom, refs, pb = ensemble.trace_opd(px, py, self.cells, planes=maps)
        self.moments = mom.cpu().numpy().reshape(K, F, W, _capi.OPD_MOMENTS)
        self.references = refs.cpu().numpy().reshape(K, F, W, -1)
        self.planar = bool(planar)
        self.opd = self.intensity = None
        if maps:
            host = pb[..., :n].cpu().numpy().reshape(K, F, W, 2, n)
            self.opd, self.intensity = host[..., 0, :], host[..., 1, :]

    def rms(self) -> np.ndarray:
        """(K, F, W): sqrt(mean(opd^2)) in waves over the rays that arrive (`OPD.rms`)."""
        return opd_statistics(self.moments)[0]

    def mean(self) -> np.ndarray:
        """(K, F, W): mean OPD in waves over the rays that arrive."""
        return opd_statistics(self.moments)[1]

    @property
    def radius(self) -> np.ndarray:
        """(K, F, W): radius of every cell's reference sphere in mm (inf for plane references)."""
        if self.planar:
            return np.full(self.moments.shape[:3], np.inf)
        return self.references[..., 3]
