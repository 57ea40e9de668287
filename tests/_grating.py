"""What the diffraction-grating tests share (tests/test_grating_cpu.py, tests/test_gpu_grating.py)
and what tools/make_golden_grating.py builds its fixture from: the lenses of the reference's
tests/test_grating.py and their variants, the fixture tests/golden/grating.npz, the bounds, the
case files of tests/hostgrating and the CPU stand-in engine of the drop-in test.

Bounds (the project's contract, nothing taken from what the code gives).
  * positions and the optical path: 1e-6 (fp64) / 1e-4 (fp32) of the system scale -- the largest
    finite |x|, |y|, |z| or opd of the case's reference rows, at least 1;
  * direction cosines and the intensity: 1e-6 / 1e-4 absolute;
  * fp64 also at the 1e-12 the README states for conic-only systems (positions: of the scale);
  * a ray that is NaN in the reference is NaN here, and no other; intensity 0 likewise.
The fixture holds no ray with |S| / n2^2 < 1e-2 (S = n2^2 - |T|^2, the radicand of the grating
equation): near S = 0 the direction is ill conditioned -- d k / d S ~ 1 / sqrt(S) -- and the NaN
mask would depend on rounding.  The generator drops such rays; `radicand` below recomputes S from
the table and the recorded rows and the tests assert the margin on the fixture.
"""

from __future__ import annotations

import functools
import importlib.util
import os
import subprocess

import numpy as np

from optiland_amd import system as S
from optiland_amd.system import SystemTable

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "grating.npz")
MAGIC = int.from_bytes(b"olGRAT", "little")

WAVELENGTH = 0.587
CONTRACT = {np.float64: 1e-6, np.float32: 1e-4}
TIGHT = 1e-12
MARGIN = 1e-2                  # |S| / n2^2 of every fixture ray is at least this
BIG_SET = "disc1027"
BIG_CASES = ("conic_t", "evan_m1")

# name -> (base lens, keyword edits of the grating surface, Hy of the hexapolar set)
CASES = {
    "flat_t": ("flat", {}, 1.0),
    "conic_t": ("conic", {}, 1.0),
    "conic_r": ("mirror", {}, 1.0),
    "flat_angle": ("flat", dict(groove_orientation_angle=0.6), 1.0),
    "conic_angle": ("conic", dict(groove_orientation_angle=0.6), 1.0),
    "mirror_angle": ("mirror", dict(groove_orientation_angle=0.6), 1.0),
    "flat_m2": ("flat", dict(grating_order=-2), 1.0),
    "conic_0": ("conic", dict(grating_order=0), 1.0),
    "flat_p1": ("flat", dict(grating_order=1), 1.0),
    "glass": ("glass", {}, 1.0),
    "tilted": ("conic", dict(rx=0.03, dy=0.4, groove_orientation_angle=0.6), 1.0),
    "clipped": ("conic", dict(aperture=7.0), 1.0),
    "coated_t": ("flat", dict(coating=(0.9, 0.05)), 1.0),
    "coated_r": ("mirror", dict(coating=(0.9, 0.05)), 1.0),
    # a NEGATIVE period: the reference's root term changes sign with it (sqrt(d^2 S) / d), the
    # ray leaves on the other side of the surface -- not the same as the opposite order
    "negative_t": ("conic", dict(grating_period=-5.0, grating_order=1), 1.0),
    "negative_flat": ("flat", dict(grating_period=-5.0, groove_orientation_angle=0.6), 1.0),
    "negative_r": ("mirror", dict(grating_period=-5.0), 1.0),
    "evan_m1": ("conic", dict(grating_period=0.7, grating_order=-1), -1.0),
    "evan_p1": ("conic", dict(grating_period=0.7, grating_order=1), 1.0),
}
# the reference's own known answers (its tests/test_grating.py): lens, (Hx, Hy, Px, Py), (L, M, N)
KNOWN = (
    ("flat", (0.0, 0.0, 0.0, 0.0), (0.0, -0.1174, 0.9930847094)),
    ("flat", (0.0, 0.0, 0.0, 1.0), (0.0, -0.1174, 0.9930847094)),
    ("flat", (0.2, 0.8, -0.15, 0.7), (0.0345602649, 0.0216899611, 0.9991672201)),
    ("conic", (0.0, 0.0, 0.0, 0.0), (0.0, -0.1174, 0.9930847094)),
    ("conic", (0.0, 0.0, 0.0, 1.0), (0.0, -0.0379603895, 0.9992792447)),
    ("conic", (0.2, 0.8, -0.15, 0.7), (0.0229384233, 0.0764682608, 0.9968081229)),
    ("mirror", (0.2, 0.8, -0.15, 0.7), (-0.0040370331, -0.4006582284, 0.9162186892)),
)


# ------------------------------------------------------------------ the lenses (need the reference)
def lens(base: str, **edit):
    """The three lenses of the reference's tests/test_grating.py -- "flat" (plane transmission
    grating behind an N-BK7 plate), "conic" (the same with R 50, k 1), "mirror" (reflective, R 70)
    -- and "glass" (the conic grating between N-BK7 and N-SF11, one more surface back to air), with
    keyword edits of the grating surface.  `aperture`: r_max of a RadialAperture; `coating`:
    (transmittance, reflectance) of a SimpleCoating.  Built on the ACTIVE backend."""
    import optiland.backend as be
    from optiland.coatings import SimpleCoating
    from optiland.optic import Optic
    from optiland.physical_apertures import RadialAperture

    if "aperture" in edit:
        edit["aperture"] = RadialAperture(r_max=edit["aperture"])
    if "coating" in edit:
        edit["coating"] = SimpleCoating(*edit["coating"])
    out = Optic(name=f"grating_{base}")
    out.surfaces.add(index=0, radius=be.inf, thickness=be.inf)
    kw = dict(surface_type="grating", grating_order=-1, grating_period=5.0,
              groove_orientation_angle=0.0, is_stop=True)
    if base == "mirror":
        kw.update(index=1, radius=70.0, thickness=-30.0, material="mirror", grating_order=1)
        kw.update(edit)
        out.surfaces.add(**kw)
        out.surfaces.add(index=2)
    else:
        out.surfaces.add(index=1, radius=be.inf, thickness=10.0)
        out.surfaces.add(index=2, radius=be.inf, thickness=5.0, material="N-BK7")
        kw.update(index=3, radius=be.inf, thickness=30.0)
        if base in ("conic", "glass"):
            kw.update(radius=50.0, conic=1.0)
        if base == "glass":
            kw.update(material="N-SF11", thickness=6.0)
        kw.update(edit)
        out.surfaces.add(**kw)
        if base == "glass":
            out.surfaces.add(index=4, radius=-80.0, thickness=24.0)
            out.surfaces.add(index=5)
        else:
            out.surfaces.add(index=4)
    out.set_aperture(aperture_type="EPD", value=15)
    out.fields.set_type(field_type="angle")
    out.fields.add(y=0)
    out.fields.add(y=10)
    out.fields.add(y=0, x=10)
    out.wavelengths.add(value=WAVELENGTH, is_primary=True)
    return out


def case_lens(name: str):
    base, edit, _hy = CASES[name]
    return lens(base, **dict(edit))


def grating_index(base: str) -> int:
    return 1 if base == "mirror" else 3


def pupil_points(rayset: str):
    """(Px, Py): the 6-ring hexapolar pupil (127 rays: one full and one partial wave) or 1027
    points uniform over the disc."""
    if rayset == "hex127":
        px, py = [0.0], [0.0]
        for ring in range(1, 7):
            th = 2.0 * np.pi * np.arange(6 * ring) / (6 * ring)
            px.extend((ring / 6.0) * np.cos(th))
            py.extend((ring / 6.0) * np.sin(th))
        return np.array(px), np.array(py)
    rng = np.random.default_rng(1027)
    r, th = np.sqrt(rng.uniform(0.0, 1.0, 1027)), rng.uniform(0.0, 2.0 * np.pi, 1027)
    return r * np.cos(th), r * np.sin(th)


def packed(optic) -> SystemTable:
    """The tolerant pack the drop-in's bridge makes of the lens' surfaces for an engine that
    traces gratings."""
    from optiland_amd.packer import pack_surfaces

    return pack_surfaces(optic.surfaces.surfaces, [WAVELENGTH], name=optic.name, tolerate=True,
                         gratings=True)


# ------------------------------------------------------------------ the grating equation in NumPy
def radicand(table: SystemTable, g: int, before: np.ndarray, after: np.ndarray) -> np.ndarray:
    """S / n2^2 per ray of the grating row `g`: from the state in front of the surface (8, n) and
    the recorded hit behind it (8, n), both in the global frame.  Written from the reference's
    definitions (surface_normal, _tangent, grating_vector, the period correction), not from the
    kernel: the fixture's margin is judged by it."""
    row = table.surfaces[g]
    R = np.asarray(row["rot"], dtype=np.float64).reshape(3, 3)
    p = R @ (after[:3] - np.asarray(row["origin"], dtype=np.float64)[:, None])
    k0 = R @ before[3:6]
    off = int(row["coeff_offset"])
    order, period, angle = (float(v) for v in table.coeffs[off:off + 3])
    n1, n2 = float(table.optics["n1"][g, 0]), float(table.optics["n2"][g, 0])
    x, y = p[0], p[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        if int(row["geom_kind"]) == S.GEOM_PLANE_GRATING:
            n = np.stack([np.zeros_like(x), np.zeros_like(x), np.ones_like(x)])
            f = np.stack([-np.sin(angle) * np.ones_like(x), np.cos(angle) * np.ones_like(x),
                          np.zeros_like(x)])
        else:
            rad, k = float(row["radius"]), float(row["conic"])
            r2 = x * x + y * y
            root = np.sqrt(1.0 - (1.0 + k) * r2 / rad ** 2)
            fx, fy = x / (rad * root), y / (rad * root)
            n = np.stack([fx, fy, -np.ones_like(x)]) / np.sqrt(fx * fx + fy * fy + 1.0)
            dzdx = (x + y * np.tan(angle)) * (2 * rad ** 2 * root * (root + 1) + (k + 1) * r2) \
                / (rad ** 3 * root * (root + 1) ** 2)
            t = np.stack([np.ones_like(x), np.tan(angle) * np.ones_like(x), dzdx])
            c = np.cross(n.T, t.T).T
            f = -c / np.linalg.norm(c, axis=0)
        dot = (k0 * n).sum(axis=0)
        gq = order * float(table.wavelengths[0]) / (period / np.hypot(f[0], f[1]))
        T = n1 * (k0 - dot * n) + gq * (f - (f * n).sum(axis=0) * n)
        return (n2 * n2 - (T * T).sum(axis=0)) / (n2 * n2)


# ------------------------------------------------------------------ the fixture
@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def case_names():
    return [str(c) for c in golden()["cases"]]


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """One case: `table`, `g` (the grating row), `rows` (S + 1, 8, n) -- what every surface
    recorded of the reference's `Optic.trace` on the NumPy backend, row 0 the object surface's --
    and, in the BIG_CASES, `big_in` / `big_out` (8, 1027 or fewer): the state in front of the
    grating and its recorded row for the big ray set.  Treat as read-only."""
    gd = golden()
    out = {k.split("/", 1)[1]: gd[k] for k in gd if k.startswith(name + "/")}
    out["name"] = name
    out["table"] = SystemTable.from_json(str(out["table"]))
    out["g"] = int(out["g"])
    for k in ("rows", "big_in", "big_out"):
        if k in out:
            out[k].setflags(write=False)
    return out


def scale_of(rows: np.ndarray) -> float:
    """The system scale of a case: the largest finite position or path length, at least 1."""
    v = np.abs(rows[..., [0, 1, 2, 7], :])
    v = v[np.isfinite(v)]
    return max(1.0, float(v.max()) if v.size else 1.0)


def bounds(dtype, scale: float, tight: bool = False) -> np.ndarray:
    """(8, 1): the bound of every plane (x y z L M N intensity opd)."""
    b = TIGHT if tight else CONTRACT[dtype]
    return np.array([b * scale] * 3 + [b] * 4 + [b * scale])[:, None]


def compare(got: np.ndarray, want: np.ndarray, dtype, scale: float, what: str, tight: bool = False,
            report=None) -> float:
    """`got` against `want` (..., 8, n): the NaN masks, the i == 0 masks, then every plane within
    its bound.  Returns the worst error as a share of its bound."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN mask differs"
    assert np.array_equal(got[..., 6, :] == 0, want[..., 6, :] == 0), f"{what}: i == 0 mask differs"
    lim = bounds(dtype, scale, tight)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    err = np.where(np.isnan(err), 0.0, err)
    ratio = float((err / lim).max()) if err.size else 0.0
    if report is not None:
        report(f"{what} {np.dtype(dtype).name}{' tight' if tight else ''}: worst error / bound = "
               f"{ratio:.3g} (worst error {float(err.max()) if err.size else 0.0:.3g})")
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ------------------------------------------------------------------ tests/hostgrating
def _builder():
    spec = importlib.util.spec_from_file_location(
        "_hostgrating_build", os.path.join(HERE, "hostgrating", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sanitizers_available(tmp_dir) -> bool:
    """Whether THIS box can build and run a program with AddressSanitizer +
    UndefinedBehaviorSanitizer at all: a trivial program through the compiler and the flags the
    checker's sanitized build uses.  The only reason to skip the sanitized test; a failure to build
    the checker itself where this succeeds is a failure."""
    import shutil

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin",
                         "clang++")
    if not os.path.exists(clang):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
    src, exe = os.path.join(str(tmp_dir), "probe.cpp"), os.path.join(str(tmp_dir), "probe")
    with open(src, "w") as f:
        f.write("#include <vector>\nint main() { std::vector<int> v(3, 1); return v[0] + v[2] - 2; }\n")
    try:
        subprocess.run([clang, "-fsanitize=address,undefined", src, "-o", exe], check=True,
                       capture_output=True, timeout=120)
        return subprocess.run([exe], capture_output=True, timeout=60).returncode == 0
    except (OSError, subprocess.SubprocessError):
        return False


def write_case(path, table: SystemTable, planes, surface: int, fp64: bool = True,
               wavelength: float | None = None) -> None:
    """The flat file tests/hostgrating/main.hip reads (its header comment has the layout)."""
    surf = np.ascontiguousarray(table.surfaces)
    optics = np.ascontiguousarray(table.optics)
    coeffs = np.ascontiguousarray(table.coeffs, dtype=np.float64)
    planes = np.ascontiguousarray(planes, dtype="<f8")
    assert planes.shape[0] == 8
    head = np.array([MAGIC, surf.shape[0], optics.shape[1], coeffs.size, planes.shape[1], surface,
                     0, int(fp64)], dtype="<i8")
    wl = np.array([float(table.wavelengths[0]) if wavelength is None else wavelength], dtype="<f8")
    with open(path, "wb") as f:
        for a in (head, wl, surf, optics, coeffs, planes):
            f.write(np.ascontiguousarray(a).tobytes())


def run_host(exe: str, mode: str, path) -> str:
    done = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (done.returncode, done.stdout[-400:], done.stderr[-400:])
    return done.stdout


def host_step(exe: str, path):
    """(8, n) of `hostgrating step`, and the OR of the rays' status bits."""
    out, bits = [], 0
    for line in run_host(exe, "step", path).splitlines():
        part = line.split()
        assert part[0] == "ray", line
        out.append([float(v) for v in part[2:10]])
        bits |= int(part[10])
    return np.array(out, dtype=np.float64).reshape(-1, 8).T.copy(), bits


# ------------------------------------------------------------------ CPU stand-in of the engine
def make_engine_class(exe: str, tmp_dir):
    """`OracleEngine` (tests/_fake_engine.py) for the fused runs + the host checker for the grating
    rows, joined by the product's own splitter (`optiland_amd.engine.split_trace`): what
    `HipSystem.trace` does on a range with grating rows, on CPU tensors."""
    from tests._fake_engine import single_kind_engine_class

    def step(engine, planes, surface, wavelength_index):
        path = os.path.join(str(tmp_dir), f"engine_{id(engine)}.case")
        write_case(path, engine.table, planes, surface=surface,
                   wavelength=float(engine.table.wavelengths[wavelength_index]))
        return host_step(exe, path)[0]

    return single_kind_engine_class(S.KIND_GRATING, step)
