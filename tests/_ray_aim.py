"""What the ray-aiming tests share (tests/test_ray_aim_cpu.py, tests/test_gpu_ray_aim.py): the
fixture tests/golden/ray_aim.npz (tools/make_golden_ray_aim.py), the bounds derived from it, and
the case files of tests/hostaim.

Bounds.  Two launch states that both put a ray within `tol` of its target on the stop plane are
at most 2 tol apart THERE, hence -- to first order -- at most 2 tol |J^-1| apart in the unknowns,
J the map's Jacobian at the solution (the fixture's central difference; |.| the spectral norm).
That is the floor, per ray.  Above it stands the project's usual bound, three times the spread
between the reference's own NumPy and torch results for the case.  The same figure bounds the
image-plane hits of the trace that follows (their own NumPy-to-torch spread taken instead).
"""

from __future__ import annotations

import functools
import importlib.util
import os

import numpy as np

from optiland_amd.system import SystemTable

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ray_aim.npz")
MAGIC = int.from_bytes(b"olAIM", "little")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def cases():
    return [str(c) for c in golden()["cases"]]


@functools.lru_cache(maxsize=None)
def table(system: str) -> SystemTable:
    return SystemTable.from_json(str(golden()[f"{system}/table"]))


def case(name: str) -> dict:
    g = golden()
    out = {k.split("/", 1)[1]: g[k] for k in g if k.startswith(name + "/")}
    out["system"] = str(out["system"])
    for k in ("hy", "wavelength", "tol", "r_stop", "jacobian"):
        out[k] = float(out[k])
    for k in ("max_iter", "first", "stop", "passes", "solves"):
        out[k] = int(out[k])
    out["infinite"] = bool(out["infinite"])
    out["table"] = table(out["system"])
    return out


def floor(c: dict) -> np.ndarray:
    """2 tol |J^-1| per ray."""
    inv = np.linalg.inv(c["fd_jacobian"])
    return 2.0 * c["tol"] * np.linalg.norm(inv, ord=2, axis=(1, 2))


def launch_bound(c: dict) -> np.ndarray:
    spread = float(np.max(np.abs(c["solved"] - c["torch_solved"])))
    return np.maximum(3.0 * spread, floor(c))


def image_bound(c: dict) -> np.ndarray:
    spread = float(np.max(np.abs(c["image"][:3] - c["torch_image"][:3])))
    return np.maximum(3.0 * spread, floor(c))


def contract_slack(c: dict, lx, ly) -> np.ndarray:
    """8 ulp of max(|x|, |y|, r_stop): the frame round trip of a re-trace."""
    return 8.0 * np.spacing(np.maximum(np.maximum(np.abs(lx), np.abs(ly)), abs(c["r_stop"])))


def stop_local(tab: SystemTable, stop: int, x, y, z):
    """Global coordinates -> the stop surface's frame (its packed origin and rotation)."""
    row = tab.surfaces[stop]
    R = np.asarray(row["rot"], dtype=np.float64).reshape(3, 3)
    d = np.stack([x, y, z]) - np.asarray(row["origin"], dtype=np.float64)[:, None]
    return R @ d


# ------------------------------------------------------------------ tests/hostaim
def _builder():
    spec = importlib.util.spec_from_file_location(
        "_hostaim_build", os.path.join(HERE, "hostaim", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_case(path, c: dict, *, use_guess: bool, max_iter=None, guess=None, n=None):
    """The flat file tests/hostaim/main.hip reads (its header comment has the layout)."""
    tab = c["table"]
    rg = tab.raygen
    n = c["pupil"].shape[1] if n is None else n
    surf = np.ascontiguousarray(tab.surfaces)
    optics = np.ascontiguousarray(tab.optics)
    coeffs = np.ascontiguousarray(tab.coeffs, dtype=np.float64)
    head = np.array([MAGIC, surf.shape[0], optics.shape[1], coeffs.size, n, c["first"], c["stop"],
                     0, c["max_iter"] if max_iter is None else max_iter, int(c["infinite"]),
                     int(use_guess), 0], dtype="<i8")
    scal = np.array([c["r_stop"], c["jacobian"], c["tol"]], dtype="<f8")
    gen = np.array([rg["object_infinite"], rg.get("field_kind", 0), rg["EPL"], rg["EPD"],
                    rg.get("field_scale", rg["max_field"]), rg["offset"], rg["z_first"],
                    rg.get("tele_dz", 0.0), rg.get("apod_a", 0.0), rg.get("apod_b", 0.0),
                    rg.get("apod_kind", 0)], dtype="<f8")
    uni = np.array([0.0, c["hy"], 1.0, 1.0], dtype="<f8")
    g = c["guess"] if guess is None else guess
    with open(path, "wb") as f:
        for a in (head, scal, gen, uni, surf, optics, coeffs, c["pupil"][0][:n], c["pupil"][1][:n]):
            f.write(np.ascontiguousarray(a).tobytes())
        if use_guess:
            f.write(np.ascontiguousarray(g[:, :n], dtype="<f8").tobytes())


def parse_solution(text: str):
    """(solved (6, n), updates (n,), per-ray bits (n,), status word) of `hostaim solve`."""
    rays, status = [], None
    for line in text.splitlines():
        part = line.split()
        if part[0] == "ray":
            rays.append([float(v) for v in part[2:8]] + [int(part[8]), int(part[9])])
        elif part[0] == "status":
            status = int(part[1])
        else:
            raise AssertionError(f"hostaim: {line}")
    a = np.array(rays, dtype=np.float64).reshape(-1, 8)
    return a[:, :6].T.copy(), a[:, 6].astype(np.int32), a[:, 7].astype(np.uint32), status
