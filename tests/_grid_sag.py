"""What the grid-sag tests share (tests/test_grid_sag_cpu.py, tests/test_gpu_grid_sag.py) and what
tools/make_golden_grid_sag.py builds its fixture from: a singlet (object, stop, the grid-sag front
surface, a spherical back surface, image) whose front surface is the reference's GridSagGeometry
-- a sampled sphere plus a smooth ripple --, the fixture tests/golden/grid_sag.npz, the bounds, the
case files of tests/hostgrid and the cell choice written from the reference's definition.

Bounds (`compare`, `bounds`, `scale_of` are tests/_grating.py's): at tol = 1e-12 fp64 within 1e-12;
at the factory's tol = 1e-6 the contract, 1e-6 (fp64) / 1e-4 (fp32) -- there the reference stops
the whole batch at once and a ray of its own may have taken fewer updates --, positions and path
lengths relative to the system scale, NaN masks equal.

What the fixture holds, and what it does not: each case is traced at ONE field, 0 or 1 (they
alternate over the cases: six at field 1, five at field 0), not at both, and the clipped, coated
and 2 x 2 cases with 127 rays instead of 469 -- both tolerances of all eleven cases at ~470 rays
and two fields do not fit the size limit of a committed file (the fixture is 0.84 MB as it is).
The hexapolar sets are turned by HEX_TURN (below).
"""

from __future__ import annotations

import functools
import importlib.util
import os

import numpy as np

from optiland_amd import system as S
from optiland_amd.system import SystemTable
from tests._grating import (CONTRACT, TIGHT, bounds, compare, run_host,  # noqa: F401
                            sanitizers_available, scale_of)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "grid_sag.npz")
MAGIC = int.from_bytes(b"olGRID", "little")

WAVELENGTH = 0.587
GRID = 2                       # the grid-sag row of every case: object, stop, grid, back, image
TOLS = {"tight": 1e-12, "factory": 1e-6}
RESIDUAL = 1e-13               # |sag(x, y) - z| at the reference's hit, every ray that is not NaN
# The slope of the interpolant jumps across a grid line, so a hit within rounding of one -- the
# hexapolar ray at 5 cos(60 deg) = 2.5000000000000004 beside the node 2.5 -- is in another cell
# once its coordinate is rounded to float.  The ray sets are turned by HEX_TURN so that no such
# ray exists: every hit is EXACTLY on a grid line (the chief ray's x = 0, the nodes case) or at
# least LINE_MARGIN millimetres from the nearest (fp32 hits are good to ~1e-6).  The generator
# asserts it and so does the CPU suite.
LINE_MARGIN = 2e-5
HEX_TURN = 0.1

# name -> (keyword edits of `lens`, (Hx, Hy), ray set)
CASES = {
    "uniform": (dict(), (0.0, 1.0), "hex469"),                       # 33 x 29
    "coarse": (dict(nx=5, ny=7), (0.0, 0.0), "hex469"),
    "nonuniform": (dict(spacing=1.3), (0.0, 1.0), "hex469"),
    "tilted": (dict(rx=0.03, ry=-0.02, dx=0.5, dy=-0.3), (0.0, 0.0), "hex469"),
    "mirror": (dict(material="mirror"), (0.0, 1.0), "hex469"),
    "concave": (dict(radius=-20.0), (0.0, 0.0), "hex469"),
    "narrow": (dict(half=4.6), (0.0, 1.0), "hex469"),                # part of the bundle leaves
    "clipped": (dict(aperture=4.0), (0.0, 1.0), "hex127"),
    "coated": (dict(coating=(0.9, 0.05)), (0.0, 0.0), "hex127"),
    # the reference's own test plane (tests/test_grid_sag_geometry.py): sag = 0.1 x on [-1, 1]^2
    "plane2x2": (dict(plane=True, epd=1.6), (0.0, 0.0), "hex127"),
    # rays through exact node coordinates and along exact cell borders (33 x 33: pitch 0.5, binary
    # numbers, and so are the pupil coordinates m / 8 of an EPD of 8)
    "nodes": (dict(ny=33, epd=8.0), (0.0, 0.0), "nodes"),
}
NAN_CASES = ("narrow",)


def hexapolar(rings: int):
    px, py = [0.0], [0.0]
    for ring in range(1, rings + 1):
        th = HEX_TURN + 2.0 * np.pi * np.arange(6 * ring) / (6 * ring)
        px.extend((ring / rings) * np.cos(th))
        py.extend((ring / rings) * np.sin(th))
    return np.array(px), np.array(py)


def pupil_points(rayset: str):
    """(Px, Py): 12 rings (469 rays), 6 rings (127), or pupil points that put the rays of the
    on-axis field (collimated along z, EPD 8) on nodes and cell borders of the 0.5 mm grid."""
    if rayset == "hex469":
        return hexapolar(12)
    if rayset == "hex127":
        return hexapolar(6)
    assert rayset == "nodes", rayset
    k = np.arange(-6, 7) / 8.0                 # x = -3 .. 3 in steps of the pitch
    on_nodes = [(a, b) for a in k[::2] for b in k[::2]]
    on_x_border = [(a, 0.123 + 0.05 * i) for i, a in enumerate(k)]
    on_y_border = [(-0.377 + 0.04 * i, b) for i, b in enumerate(k)]
    p = np.array(on_nodes + on_x_border + on_y_border)
    return p[:, 0].copy(), p[:, 1].copy()


# ------------------------------------------------------------------ the grids
def axis(half: float, n: int, spacing: float = 1.0) -> np.ndarray:
    """n coordinates over [-half, half]: uniform, or sign(u) |u|^spacing of uniform u."""
    u = np.linspace(-1.0, 1.0, n)
    return half * np.sign(u) * np.abs(u) ** spacing


def sag_table(xs, ys, radius: float) -> np.ndarray:
    """A sphere of the given radius plus a smooth ripple, sampled at the nodes: (H, W)."""
    x, y = xs[None, :], ys[:, None]
    r2 = x * x + y * y
    sphere = r2 / (radius * (1.0 + np.sqrt(1.0 - r2 / radius ** 2)))
    return sphere + 2e-3 * np.cos(0.9 * x) * np.sin(0.7 * y + 0.3)


def grid(**edit):
    """(xs, ys, sag (H, W)) of a case."""
    if edit.get("plane"):
        xs = ys = np.array([-1.0, 1.0])
        return xs, ys, np.array([[-0.1, 0.1], [-0.1, 0.1]])
    half = edit.get("half", 8.0)
    xs = axis(half, edit.get("nx", 33), edit.get("spacing", 1.0))
    ys = axis(half, edit.get("ny", 29), edit.get("spacing", 1.0))
    return xs, ys, sag_table(xs, ys, edit.get("radius", 30.0))


# ------------------------------------------------------------------ the optics (need the reference)
def lens(tol: float = 1e-6, **edit):
    """Object, stop, the grid-sag surface, a spherical back surface, image.  Keyword edits:
    `material` ("mirror": reflecting, no back surface power), `rx` / `ry` / `dx` / `dy`,
    `aperture` (r_max of a RadialAperture), `coating` (transmittance, reflectance of a
    SimpleCoating), `epd`, everything else goes to `grid`."""
    import optiland.backend as be
    from optiland.coatings import SimpleCoating
    from optiland.optic import Optic
    from optiland.physical_apertures import RadialAperture

    edit = dict(edit)
    material = edit.pop("material", "N-BK7")
    kw = dict(index=2, surface_type="grid_sag", material=material,
              thickness=-4.0 if material == "mirror" else 4.0, tol=tol)
    for k in ("rx", "ry", "dx", "dy"):
        if k in edit:
            kw[k] = edit.pop(k)
    if "aperture" in edit:
        kw["aperture"] = RadialAperture(r_max=edit.pop("aperture"))
    if "coating" in edit:
        kw["coating"] = SimpleCoating(*edit.pop("coating"))
    epd = edit.pop("epd", 10.0)
    xs, ys, z = grid(**edit)
    out = Optic(name="grid_sag_singlet")
    out.surfaces.add(index=0, radius=be.inf, thickness=be.inf)
    out.surfaces.add(index=1, radius=be.inf, thickness=5.0, is_stop=True)
    out.surfaces.add(x_coordinates=xs.tolist(), y_coordinates=ys.tolist(), sag_values=z.tolist(),
                     **kw)
    if material == "mirror":
        out.surfaces.add(index=3, radius=be.inf, thickness=-20.0)
    else:
        out.surfaces.add(index=3, radius=-60.0, thickness=40.0)
    out.surfaces.add(index=4)
    out.set_aperture(aperture_type="EPD", value=epd)
    out.fields.set_type(field_type="angle")
    out.fields.add(y=0)
    out.fields.add(y=2)
    out.wavelengths.add(value=WAVELENGTH, is_primary=True)
    return out


def case_lens(name: str, tol: float = 1e-6):
    return lens(tol, **dict(CASES[name][0]))


def packed(optic) -> SystemTable:
    """The tolerant pack the drop-in's bridge makes of the lens' surfaces for an engine that
    traces grid-sag surfaces."""
    from optiland_amd.packer import pack_surfaces

    return pack_surfaces(optic.surfaces.surfaces, [WAVELENGTH], name=optic.name, tolerate=True,
                         grid_sags=True)


# ------------------------------------------------------------------ the interpolant in NumPy
def block_of(table: SystemTable, g: int = GRID):
    """(xs, ys, sag (H, W)) of the public block of row `g`."""
    off, n = int(table.surfaces["coeff_offset"][g]), int(table.surfaces["n_coeff"][g])
    b = np.asarray(table.coeffs[off:off + n], dtype=np.float64)
    W, H = int(b[0]), int(b[1])
    assert b.size == 2 + W + H + W * H
    return b[2:2 + W], b[2 + W:2 + W + H], b[2 + W + H:].reshape(H, W)


def cell_numpy(v: np.ndarray, x) -> np.ndarray:
    """grid_sag.py:66-79: searchsorted(side="right") - 1, then the two clamps."""
    i = np.searchsorted(v, x, side="right") - 1
    i = np.where(i < 0, 0, i)
    return np.where(i >= len(v) - 1, len(v) - 2, i)


def sag_numpy(xs, ys, z, x, y):
    """grid_sag.py:61-101 written out: (sag, ds/dx, ds/dy), NaN sag outside the grid."""
    i, j = cell_numpy(xs, x), cell_numpy(ys, y)
    x1, x2, y1, y2 = xs[i], xs[i + 1], ys[j], ys[j + 1]
    z11, z12, z21, z22 = z[j, i], z[j, i + 1], z[j + 1, i], z[j + 1, i + 1]
    tx, ty = (x - x1) / (x2 - x1), (y - y1) / (y2 - y1)
    sag = (z11 * (1 - tx) + z12 * tx) * (1 - ty) + (z21 * (1 - tx) + z22 * tx) * ty
    fx = ((z12 - z11) * (1 - ty) + (z22 - z21) * ty) / (x2 - x1)
    fy = ((z21 - z11) * (1 - tx) + (z22 - z12) * tx) / (y2 - y1)
    out = (x < xs[0]) | (x > xs[-1]) | (y < ys[0]) | (y > ys[-1])
    return np.where(out, np.nan, sag), fx, fy


def local_point(table: SystemTable, g: int, rows8: np.ndarray) -> np.ndarray:
    """(3, n): the recorded positions (8, n) in the frame of row `g`."""
    row = table.surfaces[g]
    R = np.asarray(row["rot"], dtype=np.float64).reshape(3, 3)
    return R @ (rows8[:3] - np.asarray(row["origin"], dtype=np.float64)[:, None])


def residual(table: SystemTable, g: int, after: np.ndarray) -> np.ndarray:
    """|sag(x, y) - z| at the recorded hits (8, n); NaN for a NaN ray."""
    p = local_point(table, g, after)
    with np.errstate(invalid="ignore"):
        sag, _fx, _fy = sag_numpy(*block_of(table, g), np.nan_to_num(p[0]), np.nan_to_num(p[1]))
        return np.abs(sag - p[2])


def grid_line_distance(table: SystemTable, g: int, after: np.ndarray) -> np.ndarray:
    """(2, n): distance in millimetres of the recorded hits (8, n) to the nearest grid line of
    either axis; NaN for a NaN ray."""
    xs, ys, _z = block_of(table, g)
    p = local_point(table, g, after)
    with np.errstate(invalid="ignore"):
        return np.stack([np.abs(p[0][None, :] - xs[:, None]).min(axis=0),
                         np.abs(p[1][None, :] - ys[:, None]).min(axis=0)])


# ------------------------------------------------------------------ the fixture
@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def case_names():
    return [str(c) for c in golden()["cases"]]


@functools.lru_cache(maxsize=None)
def case(name: str, tol: str = "tight") -> dict:
    """One case at one tolerance ("tight": 1e-12, "factory": 1e-6): `table` (the row's `tol` set),
    `g`, `before` (8, n: the state in front of the grid-sag surface, global frame), `after` (8, n:
    its recorded row) and `lens` (8, n: the image surface's row), the reference's NumPy backend in
    fp64.  Treat as read-only."""
    gd = golden()
    out = {"name": name, "g": GRID, "tol": TOLS[tol]}
    out["table"] = SystemTable.from_json(str(gd[f"{name}/table"]))
    out["table"].surfaces["tol"][GRID] = TOLS[tol]
    out["before"] = gd[f"{name}/before"]
    out["after"] = gd[f"{name}/{tol}/after"]
    out["lens"] = gd[f"{name}/{tol}/lens"]
    for k in ("before", "after", "lens"):
        out[k].setflags(write=False)
    return out


# ------------------------------------------------------------------ tests/hostgrid
def _builder():
    spec = importlib.util.spec_from_file_location(
        "_hostgrid_build", os.path.join(HERE, "hostgrid", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_case(path, table: SystemTable, planes, surface: int = GRID, fp64: bool = True,
               probe=None) -> None:
    """The flat file tests/hostgrid/main.hip reads (its header comment has the layout).  probe:
    coordinates for the `cells` mode, appended behind the planes."""
    surf = np.ascontiguousarray(table.surfaces)
    optics = np.ascontiguousarray(table.optics)
    coeffs = np.ascontiguousarray(table.coeffs, dtype=np.float64)
    planes = np.ascontiguousarray(planes, dtype="<f8")
    assert planes.shape[0] == 8
    probe = np.zeros(0) if probe is None else np.ascontiguousarray(probe, dtype="<f8").reshape(-1)
    head = np.array([MAGIC, surf.shape[0], optics.shape[1], coeffs.size, planes.shape[1], surface,
                     probe.size, int(fp64)], dtype="<i8")
    with open(path, "wb") as f:
        for a in (head, surf, optics, coeffs, planes, probe):
            f.write(np.ascontiguousarray(a).tobytes())


def host_step(exe: str, path):
    """(8, n) of `hostgrid step`, and the OR of the rays' status bits."""
    out, bits = [], 0
    for line in run_host(exe, "step", path).splitlines():
        part = line.split()
        assert part[0] == "ray", line
        out.append([float(v) for v in part[2:10]])
        bits |= int(part[10])
    return np.array(out, dtype=np.float64).reshape(-1, 8).T.copy(), bits


def host_cells(exe: str, path):
    """(m,), (m,): the x cell and the y cell `hostgrid cells` finds for every probe coordinate,
    each from the candidates 0, the last cell and the mean-spacing guess (they must agree: the
    program exits 1 otherwise)."""
    ix, iy = [], []
    for line in run_host(exe, "cells", path).splitlines():
        part = line.split()
        assert part[0] == "cell", line
        ix.append(int(part[2]))
        iy.append(int(part[3]))
    return np.array(ix), np.array(iy)


def table_with_grid(xs, ys, z, tol: float = 1e-12, max_iter: int = 100) -> SystemTable:
    """A three-row table -- object, a refracting grid-sag row at z = 0 (air to n = 1.5), image at
    z = 10 -- around the given grid: for block checks and the cell-choice probe, no reference
    needed."""
    desc = np.zeros(3, dtype=S.SURFACE_DESC_DTYPE)
    optics = np.zeros((3, 1), dtype=S.SURFACE_OPTICS_DTYPE)
    eye = np.eye(3).reshape(-1)
    for k in range(3):
        desc[k]["rot"] = eye
        desc[k]["radius"] = np.inf
        desc[k]["norm_radius"] = 1.0
    desc[0]["interaction"] = S.INTERACT_RECORD_ONLY
    desc[1]["interaction"] = desc[2]["interaction"] = S.INTERACT_REFRACT
    desc[2]["origin"] = (0.0, 0.0, 10.0)
    optics[0, 0] = (1.0, 1.0, 0.0)
    optics[1, 0] = (1.0, 1.5, 0.0)
    optics[2, 0] = (1.5, 1.5, 0.0)
    xs, ys, z = (np.asarray(v, dtype=np.float64) for v in (xs, ys, z))
    block = [float(xs.size), float(ys.size)] + xs.tolist() + ys.tolist() + z.reshape(-1).tolist()
    desc[1]["geom_kind"] = S.GEOM_GRID_SAG
    desc[1]["coeff_offset"] = 0
    desc[1]["n_coeff"] = len(block)
    desc[1]["tol"] = tol
    desc[1]["max_iter"] = max_iter
    return SystemTable(surfaces=desc, coeffs=np.asarray(block, dtype=np.float64), optics=optics,
                       wavelengths=np.array([WAVELENGTH]), name="grid_sag_probe")


# ------------------------------------------------------------------ CPU stand-in of the engine
def make_engine_class(exe: str, tmp_dir):
    """`OracleEngine` (tests/_fake_engine.py) for the fused runs + the host checker for the grid-sag
    rows, joined by the product's own splitter (`optiland_amd.engine.split_trace`): what
    `HipSystem.trace` does on a range with grid-sag rows, on CPU tensors."""
    from tests._fake_engine import single_kind_engine_class

    def step(engine, planes, surface, wavelength_index):
        path = os.path.join(str(tmp_dir), f"engine_{id(engine)}.case")
        write_case(path, engine.table, planes, surface=surface)
        return host_step(exe, path)[0]

    return single_kind_engine_class(S.KIND_GRID_SAG, step)
