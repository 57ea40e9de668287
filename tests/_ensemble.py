"""What the ensemble tests share (tests/test_ensemble_cpu.py, tests/test_gpu_ensemble.py) and what
tools/make_golden_ensemble.py records its fixture with: the two lenses, the six variants of each
(the reference's own `Perturbation` with fixed `ScalarSampler`s), the cells, and the readers of
tests/golden/ensemble.npz.

The fixture holds, per lens (`cooke`: conic-only, the lean kernel; `singlet`: an even asphere, the
Newton family), K = 6 variants x 2 fields x 2 wavelengths x 91 hexapolar rays, traced by the
reference on its NumPy backend:

  <lens>/tables          K packed tables (JSON text of `pack_optic`, ray-generation scalars incl.)
  <lens>/labels          what each variant perturbs
  <lens>/fields (F, 2), <lens>/wavelengths (W,), <lens>/px, <lens>/py (N,)
  <lens>/hits            (K, F, W, 3, N)  image-plane x, y, intensity of `Optic.trace`
  <lens>/operand         (K, F, W)        `RayOperand.rms_spot_size` (unmasked mean over all rays)

Variant 1 perturbs a radius IN FRONT of the stop: the entrance pupil moves, so its
ray-generation scalars are not the nominal lens's.  The decentred variant clips rays at the
aperture of the last lens surface (count < N in its cells).
"""

from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ensemble.npz")

LENSES = ("cooke", "singlet")
RINGS = 5          # 91 hexapolar points
N_RAYS = 91
# (variable type, new value, Variable kwargs) per perturbation; the VALUE is what the sampler returns
VARIANTS = {
    "cooke": (
        ("nominal", ()),
        ("radius 1 (in front of the stop)", (("radius", 22.25, dict(surface_number=1)),)),
        ("thickness 2", (("thickness", 6.15, dict(surface_number=2)),)),
        ("tilt x + decentre y of surface 6",
         (("tilt", 0.004, dict(surface_number=6, axis="x")),
          ("decenter", -0.6, dict(surface_number=6, axis="y")))),
        ("index of surface 1 at 0.55 um", (("index", 1.6245, dict(surface_number=1,
                                                                   wavelength=0.55)),)),
        ("radius 5 (behind the stop)", (("radius", 80.5, dict(surface_number=5)),)),
    ),
    "singlet": (
        ("nominal", ()),
        ("radius 1 (in front of the stop)", (("radius", 20.15, dict(surface_number=1)),)),
        ("thickness 1", (("thickness", 7.1, dict(surface_number=1)),)),
        ("tilt x + decentre y of surface 1",
         (("tilt", 0.003, dict(surface_number=1, axis="x")),
          ("decenter", 0.05, dict(surface_number=1, axis="y")))),
        ("index of surface 1 at 0.587 um", (("index", 1.79, dict(surface_number=1,
                                                                  wavelength=0.587)),)),
        ("asphere coefficient 0 of surface 1", (("asphere_coeff", -2.27e-4,
                                                  dict(surface_number=1, coeff_number=0)),)),
    ),
}
RADIUS_VARIANT = 1     # the variant whose entrance pupil moved
CLIPPED_VARIANT = 3    # (cooke) the variant that loses rays at the aperture
FIELDS = {"cooke": ((0.0, 0.0), (0.0, 0.7)), "singlet": ((0.0, 0.0), (0.0, 1.0))}
WAVELENGTHS = {"cooke": (0.48, 0.55), "singlet": (0.486, 0.587)}
# aperture of the Cooke triplet's last lens surface: just outside the nominal bundle of both
# fields (make_golden_ensemble.py asserts that, and that the decentred variant loses rays there)
COOKE_APERTURE_SURFACE, COOKE_APERTURE_RADIUS = 6, 6.5


def build_lens(name: str):
    """The reference `Optic` (current backend).  `cooke`: the reference's sample with a radial
    aperture on its last lens surface; `singlet`: the reference's aspheric singlet with the stop on
    its BACK surface (so that the front radius moves the entrance pupil), a second field and a
    second wavelength."""
    import optiland.backend as be
    from optiland import optic as optic_mod
    from optiland import physical_apertures
    if name == "cooke":
        from optiland.samples.objectives import CookeTriplet
        lens = CookeTriplet()
        lens.surfaces[COOKE_APERTURE_SURFACE].aperture = physical_apertures.RadialAperture(
            r_max=COOKE_APERTURE_RADIUS)
        return lens
    if name != "singlet":
        raise KeyError(name)
    lens = optic_mod.Optic(name="AsphericSingletBackStop")
    lens.surfaces.add(index=0, radius=be.inf, thickness=be.inf)
    lens.surfaces.add(index=1, thickness=7, radius=20.0, material="N-SF11",
                      surface_type="even_asphere", conic=0.0,
                      coefficients=[-2.248851e-4, -4.690412e-6, -6.404376e-8])
    lens.surfaces.add(index=2, thickness=21.56201105, is_stop=True)
    lens.surfaces.add(index=3)
    lens.set_aperture(aperture_type="EPD", value=16.0)
    lens.fields.set_type(field_type="angle")
    lens.fields.add(y=0)
    lens.fields.add(y=2)
    lens.wavelengths.add(value=0.486)
    lens.wavelengths.add(value=0.587, is_primary=True)
    return lens


def perturbations(optic, recipe):
    """The reference's `Perturbation` objects of one variant (fixed samplers)."""
    from optiland.tolerancing.perturbation import Perturbation, ScalarSampler
    return [Perturbation(optic, kind, ScalarSampler(value), **kw) for kind, value, kw in recipe]


# ------------------------------------------------------------------ the fixture
_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(GOLD, allow_pickle=False) as z:
            _FIX = {k: z[k] for k in z.files}
    return _FIX


def tables(lens: str):
    """The K packed tables of `lens` (fresh objects on every call)."""
    from optiland_amd.system import SystemTable
    return [SystemTable.from_json(str(s)) for s in fixture()[f"{lens}/tables"]]


def arrays(lens: str) -> dict:
    f = fixture()
    return {k.split("/", 1)[1]: f[k] for k in f if k.startswith(lens + "/") and
            not k.endswith("/tables")}


def wavelength_indices(lens: str, table) -> list:
    return [table.wavelength_index(float(w)) for w in fixture()[f"{lens}/wavelengths"]]


def operand_from_hits(x, y) -> float:
    """`RayOperand.rms_spot_size` for one wavelength (optimization/operand/ray.py:336-340): the
    unmasked mean over ALL rays, NaN included."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    r2 = (x - np.mean(x)) ** 2 + (y - np.mean(y)) ** 2
    return float(np.sqrt(np.mean(r2)))


# the project's contracts against the reference (README: accuracy), relative to the scale of the
# image-plane coordinates
def contract(lens: str, dtype_bits: int) -> float:
    if dtype_bits == 32:
        return 1e-4
    return 1e-12 if lens == "cooke" else 1e-6


# ------------------------------------------------------------------ the host program
def _builder():
    """tests/hostensemble/build.py as a module."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_hostensemble_build", os.path.join(HERE, "hostensemble", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CASE_MAGIC = 0x534e456c6f   # "olENS"


def write_case(path, tables, px, py, cells, fp64: bool) -> None:
    """A case file of tests/hostensemble/main.hip (its header comment has the layout)."""
    import ctypes as C

    from optiland_amd.ensemble import CELL_DTYPE, SystemEnsemble
    t0 = tables[0]
    cells = np.ascontiguousarray(np.asarray(cells, dtype=CELL_DTYPE).reshape(-1))
    n_coeff = int(np.asarray(t0.coeffs).size)
    with open(path, "wb") as f:
        f.write(np.array([CASE_MAGIC, len(tables), t0.num_surfaces, t0.optics.shape[1], n_coeff,
                          np.asarray(px).size, cells.size, 1 if fp64 else 0],
                         dtype="<i8").tobytes())
        for t in tables:
            coeffs = np.ascontiguousarray(t.coeffs, dtype=np.float64)
            assert coeffs.size == n_coeff, "the case file holds one coefficient count"
            f.write(np.ascontiguousarray(t.surfaces).tobytes())
            f.write(np.ascontiguousarray(t.optics).tobytes())
            f.write(coeffs.tobytes())
            rg = SystemEnsemble._raygen_params(t.raygen)
            f.write(C.string_at(C.addressof(rg), C.sizeof(rg)))
        f.write(np.ascontiguousarray(px, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(py, dtype="<f8").tobytes())
        f.write(cells.tobytes())


def run_host(mode: str, case_path: str, sanitize: bool = False):
    """One run of the host program as a child process: (lines, return code)."""
    import subprocess
    exe = _builder().build(sanitize=sanitize)
    p = subprocess.run([exe, mode, case_path], capture_output=True, text=True, timeout=120)
    return p.stdout.splitlines(), p.returncode, p.stderr


def parse_rays(lines, n_cells: int, n: int):
    """(hits (n_cells, 3, n) float64 -- NaN where a cell printed nothing --, status word)."""
    hits = np.full((n_cells, 3, n), np.nan)
    status = None
    for ln in lines:
        w = ln.split()
        if w[0] == "cell":
            hits[int(w[1]), :, int(w[3])] = [float(w[4]), float(w[5]), float(w[6])]
        elif w[0] == "status":
            status = int(w[1])
    return hits, status


# ------------------------------------------------------------------ exact truth
# Three Cooke variants x one field against tests/_exact_front.gen_ray + tests/_exact_trace.trace_ray
# at 50 digits, under `_exact_trace.bound`: twice the yardstick -- the SAME plain formulae,
# generate then trace, at the dtype's precision -- or the floor eps x scale, plus the conic-normal
# term.  Nothing here is taken from the kernels.  The nominal lens, the radius in front of the stop
# (its own entrance pupil) and the tilted, decentred surface that clips rays (its own rotated row).
EXACT_VARIANTS = (0, RADIUS_VARIANT, CLIPPED_VARIANT)
EXACT_FIELD, EXACT_WL = (0.0, 0.7), 1
EXACT_RINGS = 3        # 37 hexapolar points (+ the 5 of `_exact_trace.pupil`): seconds of mpmath
_EXACT = {}


def exact_inputs():
    """(px, py, hx, hy): numbers that are fp32 values, so both dtypes trace the same inputs."""
    from tests import _exact_front as XF
    from tests import _exact_trace as XT
    px, py = XT.pupil(EXACT_RINGS)
    return XF.f32(px), XF.f32(py), float(XF.f32(EXACT_FIELD[0])), float(XF.f32(EXACT_FIELD[1]))


def _edge_margin(table, rec):
    """Per ray the least distance of a truth hit from the edge of a radial aperture, in the row's
    own frame (inf where the table has none)."""
    from optiland_amd import system as S
    out = np.full(rec.shape[2], np.inf)
    for k, s in enumerate(table.surfaces):
        if int(s["aperture_kind"]) == S.AP_NONE:
            continue
        assert int(s["aperture_kind"]) == S.AP_RADIAL
        p = rec[k, :3] - np.asarray(s["origin"])[:, None]
        if int(s["flags"]) & S.SURF_ROTATED:
            p = np.asarray(s["rot"]).reshape(3, 3) @ p
        out = np.minimum(out, np.abs(np.hypot(p[0], p[1]) - float(s["aperture"][1])))
    return out


def exact_case(tag: str) -> dict:
    """Per variant of EXACT_VARIANTS: truth image row (8, n), keep (n,), the bound of the image
    row (4,: position, direction, path, intensity) and the edge margin (n,)."""
    if tag in _EXACT:
        return _EXACT[tag]
    from mpmath import mp

    from tests import _exact_front as XF
    from tests import _exact_trace as XT
    px, py, hx, hy = exact_inputs()
    n = px.size
    old = mp.prec
    out = {}
    try:
        for k in EXACT_VARIANTS:
            table = tables("cooke")[k]
            recs = {}
            for which, prec in (("truth", None), ("yard", XT.PREC[tag])):
                if prec is None:
                    mp.dps = 50
                else:
                    mp.prec = prec
                rec = np.full((table.num_surfaces, 8, n), np.nan)
                keep = np.zeros(n, dtype=bool)
                for j in range(n):
                    ray, _st = XF.gen_ray(mp, table.raygen, hx, hy, px[j], py[j], 1.0, 1.0, 0)
                    rows, info = XT.trace_ray(mp, table, list(ray) + [mp.mpf(0)], wl=EXACT_WL)
                    for r, row in enumerate(rows):
                        if row is not None:
                            rec[r, :, j] = [float(v) for v in row]
                    keep[j] = not (info["lost"] or info["clipped"] or info["min_cos"] < XT.MIN_COS
                                   or info["min_snell"] < XT.MIN_SNELL)
                recs[which] = (rec, keep)
            truth, keep = recs["truth"]
            assert keep.any()
            yard = XT.group_max(recs["yard"][0] - truth, keep)
            scale = XT.scales(truth, keep, table, EXACT_WL)
            znorm = XT.conic_normal_terms(table, truth, keep, EXACT_WL)
            bound = XT.bound(yard, scale, tag, np.zeros((table.num_surfaces, 4)), znorm)
            out[k] = dict(truth=truth[-1], keep=keep, bound=bound[-1],
                          margin=_edge_margin(table, truth), lit=truth[-1, 6] > 0)
    finally:
        mp.prec = old
    _EXACT[tag] = out
    return out


def exact_checks(hits, tag: str) -> list:
    """[(label, error, bound)] of `hits` {variant: (3, n) x, y, intensity} against the truth."""
    out = []
    for k, case in exact_case(tag).items():
        got = np.asarray(hits[k], dtype=np.float64)
        keep, b = case["keep"], case["bound"]
        out.append((f"variant {k} hits nan", float(np.isnan(got[:, keep]).sum()), 0.0))
        out.append((f"variant {k} position",
                    float(np.abs(got[:2, keep] - case["truth"][:2, keep]).max()), float(b[0])))
        out.append((f"variant {k} intensity",
                    float(np.abs(got[2, keep] - case["truth"][6, keep]).max()), float(b[3])))
        # whether a ray arrives, wherever the truth's hits are farther from an aperture edge than
        # the position bound
        sure = case["margin"] > b[0]
        out.append((f"variant {k} lit ({int(sure.sum())} of {sure.size} rays clear of an edge)",
                    float(((got[2] > 0) != case["lit"])[sure].sum()), 0.0))
    return out


# ------------------------------------------------------------------ the tolerancing problem
def tolerancing_problem(seed=11):
    """The reference's `Tolerancing` of the bridge tests: three `rms_spot_size` operands and four
    seeded perturbations on the Cooke triplet (the decentre clips rays in some iterations)."""
    from tests import _live
    _live.import_reference()
    from optiland.tolerancing.core import Tolerancing
    from optiland.tolerancing.perturbation import DistributionSampler
    optic = build_lens("cooke")
    tol = Tolerancing(optic)
    for hy, w in ((0.0, 0.55), (0.7, 0.55), (0.7, 0.48)):
        tol.add_operand("rms_spot_size", dict(optic=optic, surface_number=-1, Hx=0.0, Hy=hy,
                                              num_rays=5, wavelength=w, distribution="hexapolar"))
    tol.add_perturbation("radius", DistributionSampler("normal", seed=seed, loc=22.01359,
                                                       scale=0.05), surface_number=1)
    tol.add_perturbation("thickness", DistributionSampler("uniform", seed=seed + 1, low=5.9,
                                                          high=6.1), surface_number=2)
    tol.add_perturbation("decenter", DistributionSampler("normal", seed=seed + 2, loc=0.0,
                                                         scale=0.4), surface_number=6, axis="y")
    tol.add_perturbation("tilt", DistributionSampler("normal", seed=seed + 3, loc=0.0,
                                                     scale=0.002), surface_number=5, axis="x")
    return tol
