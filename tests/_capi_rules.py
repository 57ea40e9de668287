"""What the argument-rule replays share (tests/test_capi_rules_cpu.py, tests/test_gpu_capi_rules.py)
and what tools/make_golden_capi_rules.py records its fixture with: the refusals of every
system-taking C entry point, call by call.

Per entry point: the NULL system, PEELING sequences -- a call that breaks every rule that can be
broken at once with a valid system; the refusal is recorded, exactly the reported fault is
repaired, and so on until the call is accepted: every text and the order of precedence in about
as many calls as the entry has rules -- and single-fault calls for what a sequence cannot reach.
What staging refuses (ol_system_create / ol_system_update, which return at the first fault) is the
section "create": single-fault calls only (CREATE, UPDATE below).

The fixture tests/golden/capi_rules.json holds, per entry, the list of [case, return code,
ol_last_error text] ("ok" for an accepted call) as the PARENT commit of the change answered it.
Every non-NULL pointer of every call is a real buffer of N = 64 rays (NumPy arrays with the
host-math library, device tensors with the product library): a refusal that goes missing shows
as a failed comparison, and the last call of a sequence is an ordinary tiny launch.
"""

from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from optiland_amd import _capi, load_system
from optiland_amd import system as S
from optiland_amd.system import SystemTable

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "capi_rules.json")
N = 64
F32, F64 = _capi.F32, _capi.F64
OK = "ok"   # planes / structures that are given in full


def fixture() -> dict:
    with open(GOLD) as f:
        return json.load(f)


# ------------------------------------------------------------------ the systems
def _copy(table: SystemTable) -> SystemTable:
    return SystemTable.from_json(table.to_json())


def tables() -> dict:
    """name -> SystemTable: a plain lens, one with Fresnel coatings, one with a retarder, one with
    OL_SURF_REFERENCE_NEWTON on a traced Newton surface, a second lens of another size (optics_of),
    the aiming fixture's lens, the Forbes singlet plain and with a Fresnel coating, and a table
    with a grating row in front of a Forbes row (TWO_KINDS)."""
    from tests import _forbes, _ray_aim

    out = {"plain": load_system("double_gauss"), "fresnel": load_system("zernike_fresnel_fringe"),
           "other": load_system("cooke_generic"), "aim": _ray_aim.table("wa100"),
           "forbes": _forbes.case("q_norm12_default")["table"]}
    out["retarder"] = retarder_table()
    flagged = _copy(load_system("rc_asphere"))
    k = int(np.nonzero(flagged.surfaces["geom_kind"] == S.GEOM_EVEN_ASPHERE)[0][0])
    flagged.surfaces["flags"][k] |= S.SURF_REFERENCE_NEWTON
    out["newton"] = flagged
    coated = _copy(out["forbes"])
    coated.surfaces["coating_kind"][_forbes.FORBES] = S.COAT_FRESNEL
    out["forbes_coated"] = coated
    out["two_kinds"] = two_kinds_table()
    return out


def retarder_table() -> SystemTable:
    ret = _copy(load_system("double_gauss"))
    ret.coeffs = np.array([1.0, 0.0, 0.0, np.pi / 2])       # the axis and the retardance
    ret.surfaces["coating_kind"][2] = S.COAT_RETARDER
    ret.surfaces["coat"][2] = (0.0, 0.0)
    return ret


def two_kinds_table() -> SystemTable:
    """The grating fixture's table with the Forbes fixture's Forbes row appended behind it -- its
    coefficient block behind the grating's, its offset shifted: the kind that is refused LATER (the
    grating) sits at the LOWER surface index."""
    from tests import _forbes, _grating

    g, f = _copy(_grating.case("flat_t")["table"]), _forbes.case("q_norm12_default")["table"]
    assert g.optics.shape[1] == f.optics.shape[1]
    row = f.surfaces[_forbes.FORBES:_forbes.FORBES + 1].copy()
    row["coeff_offset"] += g.coeffs.size
    g.surfaces = np.concatenate([g.surfaces, row])
    g.optics = np.concatenate([g.optics, f.optics[_forbes.FORBES:_forbes.FORBES + 1]])
    g.coeffs = np.concatenate([np.asarray(g.coeffs, dtype=np.float64), f.coeffs])
    return g


def _raygen_params(table: SystemTable) -> _capi.RaygenParams:
    rg = table.raygen
    if not rg:
        return _capi.RaygenParams()
    return _capi.RaygenParams(int(rg["object_infinite"]), int(rg.get("field_kind", 0)), rg["EPL"],
                              rg["EPD"], float(rg.get("field_scale", rg["max_field"])),
                              rg["offset"], rg["z_first"], float(rg.get("tele_dz", 0.0)),
                              float(rg.get("apod_a", 0.0)), float(rg.get("apod_b", 0.0)),
                              int(rg.get("apod_kind", 0)), 0)


# ------------------------------------------------------------------ library, systems and buffers
def numpy_put(a):
    return a, a.ctypes.data


def torch_put(a):
    import torch

    t = torch.from_numpy(a).to("cuda")
    return t, t.data_ptr()


class Context:
    """A loaded library, the systems created on it and the buffers of every call.  `put` turns a
    NumPy array into (what keeps it alive, the address the library is given)."""

    def __init__(self, lib, put):
        self.lib, self._keep = lib, []
        self.tables = tables()
        self.handles = {}
        for name, t in self.tables.items():
            surf, optics = np.ascontiguousarray(t.surfaces), np.ascontiguousarray(t.optics)
            coeffs = np.ascontiguousarray(t.coeffs, dtype=np.float64)
            h = C.c_void_p()
            rc = lib.ol_system_create(surf.ctypes.data, surf.shape[0],
                                      coeffs.ctypes.data if coeffs.size else None, coeffs.size,
                                      optics.ctypes.data, optics.shape[1], C.byref(h))
            assert rc == 0, (name, lib.ol_last_error())
            self.handles[name] = h

        def buf(a):
            keep, addr = put(np.ascontiguousarray(a))
            self._keep.append(keep)
            return addr

        def planes(k):
            return [buf(np.zeros(N)) for _ in range(k)]

        g = np.arange(N, dtype=np.float64)
        px, py = 0.5 * np.cos(g) * np.sqrt(g / N), 0.5 * np.sin(g) * np.sqrt(g / N)
        rows = max(int(t.surfaces.shape[0]) for t in self.tables.values())
        # a small parallel bundle in front of the first traced surface
        self.rays = [buf(v) for v in (2.0 * px, 2.0 * py, np.full(N, -10.0), np.zeros(N),
                                      np.zeros(N), np.ones(N), np.ones(N), np.zeros(N))]
        self.px, self.py, self.field = buf(px), buf(py), buf(np.zeros(N))
        self.record = buf(np.zeros(rows * 8 * N))
        prt = np.zeros((18, N))
        prt[0] = prt[4] = prt[8] = 1.0
        self.prt = buf(prt)
        self.status = buf(np.zeros(2, dtype=np.int32))   # (the uint32 status word)
        self.iters = buf(np.zeros(2 * rows, dtype=np.int32))
        self.rays_out, self.hits, self.pupil = planes(8), planes(3), planes(3)
        self.hits_block = buf(np.zeros(2 * 3 * N))   # two cells x three planes
        self.out8 = buf(np.zeros(8 * (_capi.SPOT_BATCH_MAX_CELLS + 1)))
        self.moments = buf(np.zeros(_capi.OPD_MOMENTS))
        self.reference = buf(np.zeros(_capi.WAVEFRONT_REFERENCE_DOUBLES))
        self.chief = buf(np.zeros(8))
        self.opd, self.inten = buf(np.zeros(N)), buf(np.zeros(N))
        self.aim_out, self.aim_guess = planes(6), planes(6)
        self.updates = buf(np.zeros(N, dtype=np.int32))
        self.row = buf(np.zeros(8 * N))

    def close(self):
        for h in self.handles.values():
            self.lib.ol_system_destroy(h)
        self.handles = {}

    def handle(self, a):
        return self.handles[a["sys"]] if a["sys"] else None

    def table(self, a):
        return self.tables[a["sys"] or "plain"]


def _planes(addresses, sel):
    """`sel`: OK, None (no array at all) or the index of the one plane that is NULL."""
    if sel is None:
        return None
    arr = (C.c_void_p * len(addresses))(*addresses)
    if sel != OK:
        arr[sel] = None
    return arr


def _inputs(k: Context, a):
    """ol_raygen_inputs: `in` is OK, None, "no py", "field planes", "hx alone", "vig planes"."""
    if a["in"] is None:
        return None
    planes = {"field planes": (k.field, k.field, None, None), "hx alone": (k.field, None, None, None),
              "vig planes": (None, None, k.field, k.field)}.get(a["in"], (None,) * 4)
    return _capi.RaygenInputs(planes[0], planes[1], k.px, None if a["in"] == "no py" else k.py,
                              planes[2], planes[3], 0.0, a.get("hy0", 0.0), 1.0, 1.0,
                              a.get("in_flags", 0), 0)


def _ref(x):
    return None if x is None else C.byref(x)


def _wavefront():
    return _capi.WavefrontParams(zc=60.0, R=60.0, n_image=1.0, half_epd=5.0, wavelength_um=0.55)


# ------------------------------------------------------------------ the calls
def trace_ex(k, a):
    ex = None
    if a["extras"]:
        ex = _capi.TraceExtras(record_first_surface=a["extras"].get("record_first_surface", 0))
    return k.lib.ol_trace_ex(k.handle(a), a["dt"], a["n"], _planes(k.rays, a["rays"]), a["wl"],
                             k.record if a["record"] else None, a["stride"],
                             k.prt if a["prt"] else None, a["first"], a["last"], a["flags"],
                             k.status, _ref(ex), None)


def trace(k, a):
    return k.lib.ol_trace(k.handle(a), a["dt"], a["n"], _planes(k.rays, a["rays"]), a["wl"],
                          k.record if a["record"] else None, a["stride"],
                          k.prt if a["prt"] else None, a["first"], a["last"], a["flags"], k.status,
                          None)


def newton_count(k, a):
    return k.lib.ol_newton_count(k.handle(a), a["dt"], a["n"], _planes(k.rays, a["rays"]), a["wl"],
                                 a["first"], a["surface"], k.iters if a["iterations"] else None, 0,
                                 None)


def trace_generate(k, a):
    p, inp = _raygen_params(k.table(a)) if a["p"] else None, _inputs(k, a)
    ex = None
    if a["extras"]:
        ex = _capi.TraceExtras(record_first_surface=a["extras"].get("record_first_surface", 0))
    return k.lib.ol_trace_generate(k.handle(a), a["dt"], a["n"], _ref(p), _ref(inp), a["wl"],
                                   k.record if a["record"] else None, a["stride"],
                                   _planes(k.rays_out, a["rays_out"]), k.prt if a["prt"] else None,
                                   a["flags"], k.status, _ref(ex), None)


def trace_spot(k, a):
    p, inp = _raygen_params(k.table(a)) if a["p"] else None, _inputs(k, a)
    return k.lib.ol_trace_spot(k.handle(a), a["dt"], a["n"], _ref(p), _ref(inp), 0.0, 0.0, a["wl"],
                               _planes(k.hits, a["hits"]), k.out8 if a["out"] else None, k.status,
                               None)


def trace_spot_batch(k, a):
    p, inp = _raygen_params(k.table(a)) if a["p"] else None, _inputs(k, a)
    cells = (_capi.SpotCell * (_capi.SPOT_BATCH_MAX_CELLS + 1))()
    for c in cells:
        c.vx = c.vy = 1.0
    cells[1].wavelength_index = a["cell_wl"]
    cells[1].hy = a["cell_hy"]
    cells[1].optics_of = k.handles[a["optics_of"]] if a["optics_of"] else None
    return k.lib.ol_trace_spot_batch(k.handle(a), a["dt"], a["n"], _ref(p), _ref(inp), a["n_cells"],
                                     cells, k.hits_block if a["hits"] else None, a["stride"],
                                     k.out8 if a["out"] else None, k.status, None)


def trace_opd(k, a):
    p, inp, w = _raygen_params(k.table(a)) if a["p"] else None, _inputs(k, a), _wavefront()
    return k.lib.ol_trace_opd(k.handle(a), a["dt"], a["n"], _ref(p), _ref(inp), _ref(w), a["wl"],
                              k.opd, k.inten, _planes(k.pupil, a["pupil"]),
                              k.moments if a["moments"] else None, k.status, None)


def wavefront_reference(k, a):
    p, inp, w = _raygen_params(k.table(a)) if a["p"] else None, _inputs(k, a), _wavefront()
    return k.lib.ol_wavefront_reference(k.handle(a), a["dt"], _ref(p), _ref(inp), _ref(w), 0.0, 0,
                                        a["wl"], k.reference if a["reference"] else None, k.chief,
                                        k.status, None)


def trace_opd_dev(k, a):
    p, inp = _raygen_params(k.table(a)) if a["p"] else None, _inputs(k, a)
    return k.lib.ol_trace_opd_dev(k.handle(a), a["dt"], a["n"], _ref(p), _ref(inp), k.reference,
                                  a["wl"], k.opd, k.inten, _planes(k.pupil, a["pupil"]),
                                  k.moments if a["moments"] else None, k.status, None)


def trace_forbes(k, a):
    return k.lib.ol_trace_forbes(k.handle(a), a["dt"], a["n"], _planes(k.rays, a["rays"]), a["wl"],
                                 k.row if a["record"] else None, a["stride"], a["surface"],
                                 a["flags"], k.status, None)


def aim_rays(k, a):
    from tests import _ray_aim

    c = _ray_aim.case("wa100_h07")
    p = None
    if a["p"]:
        p = _capi.AimParams(c["r_stop"], c["jacobian"], a["tol"], a["max_iter"],
                            int(c["infinite"]), _raygen_params(k.tables["aim"]))
    return k.lib.ol_aim_rays(k.handle(a), a["n"], a["wl"], a["first"], a["stop"], _ref(p),
                             _ref(_inputs(k, a)), _planes(k.aim_guess, a["guess"]),
                             _planes(k.aim_out, a["out"]), k.updates,
                             k.status if a["status"] else None, None)


# ------------------------------------------------------------------ the cases
# a fault: (name, a piece of the text that reports it, the arguments that break the rule[, the
# arguments that repair it -- default: the entry's valid ones])
DTYPE = ("dtype", "dtype", {"dt": 7})
COUNT = ("count", "negative", {"n": -1})
WAVELENGTH = ("wavelength", "wavelength index", {"wl": 99})   # (replaced by n_wl of the system)
POLARISATION = ("polarisation", "Polarization must be set", {"prt": False}, {"prt": True})
RETARDER = ("retarder", "is a retarder", {"flags": 0}, {"flags": S.TRACE_PRT_COMPLEX})
RECORD_FROM = ("record_first_surface", "record_first_surface",
               {"extras": {"record_first_surface": 99}}, {"extras": None})


def _holes(key, count):
    return [(f"{key}[{i}] NULL", {key: i}) for i in range(count)]


def _refused_systems(*names):
    return [(f"{n} system", {"sys": n}) for n in names]


ENTRIES = {
    "ol_trace_ex": dict(
        call=trace_ex,
        valid=dict(sys="plain", dt=F64, n=N, rays=OK, wl=0, record=True, stride=N, prt=False,
                   first=0, last=12, flags=0, extras=None),
        peels={
            "plain": [DTYPE, COUNT, ("range", "surface range", {"first": 2, "last": 1}), WAVELENGTH,
                      ("plane", "rays[3]", {"rays": 3}), ("stride", "record_stride", {"stride": N - 1}),
                      RECORD_FROM],
            "fresnel": [("system", "", {"sys": "fresnel", "last": 3}, {}), POLARISATION],
            "retarder": [("system", "", {"sys": "retarder"}, {}), POLARISATION, RETARDER],
        },
        singles=[("no rays", {"n": 0}), ("first -1", {"first": -1}), ("last past the table", {"last": 13}),
                 ("wavelength -1", {"wl": -1}), ("rays NULL", {"rays": None}),
                 ("nothing to write", {"record": False}),
                 ("forbes range", {"sys": "forbes", "last": 3}),
                 ("forbes range, no rays", {"sys": "forbes", "last": 3, "n": 0}),
                 ("in front of the forbes row", {"sys": "forbes", "last": 0}),
                 ("reference newton without counts", {"sys": "newton", "last": 6})]
        + _holes("rays", 8),
        accepted=("no rays", "in front of the forbes row")),
    "ol_newton_count": dict(
        call=newton_count,
        valid=dict(sys="newton", dt=F64, n=N, rays=OK, wl=0, first=0, surface=4, iterations=True),
        peels={"newton": [DTYPE, COUNT, ("range", "surface range", {"first": 5}), WAVELENGTH,
                          ("iterations", "iterations is NULL", {"iterations": False}),
                          ("plane", "rays[3]", {"rays": 3})]},
        singles=[("no rays", {"n": 0}), ("first -1", {"first": -1}), ("surface past the table", {"surface": 7}),
                 ("wavelength -1", {"wl": -1}), ("rays NULL", {"rays": None}),
                 ("not a flagged surface", {"surface": 3}),
                 ("forbes range", {"sys": "forbes", "surface": 1})] + _holes("rays", 8),
        accepted=("no rays",)),
    "ol_trace_generate": dict(
        call=trace_generate,
        valid=dict(sys="plain", dt=F64, n=N, p=True, wl=0, record=True, stride=N, rays_out=None,
                   prt=False, flags=0, extras=None, **{"in": OK}),
        peels={
            "plain": [DTYPE, ("params", "NULL argument", {"p": False}), COUNT, WAVELENGTH,
                      ("vignetting planes", "per-ray vignetting", {"in": "vig planes"}),
                      ("record", "record is NULL", {"record": False}),
                      ("stride", "record_stride", {"stride": N - 1}), RECORD_FROM,
                      ("plane", "rays_out[3]", {"rays_out": 3})],
            "fresnel": [("system", "", {"sys": "fresnel"}, {}), POLARISATION],
            "retarder": [("system", "", {"sys": "retarder"}, {}), POLARISATION, RETARDER],
        },
        singles=[("no rays", {"n": 0}), ("wavelength -1", {"wl": -1}), ("inputs NULL", {"in": None}),
                 ("no py", {"in": "no py"}), ("hx alone", {"in": "hx alone"})]
        + _refused_systems("forbes", "newton") + _holes("rays_out", 8),
        accepted=("no rays",)),
    "ol_trace_spot": dict(
        call=trace_spot,
        valid=dict(sys="plain", dt=F64, n=N, p=True, wl=0, hits=OK, out=True, **{"in": OK}),
        peels={
            "plain": [DTYPE, ("out", "NULL argument", {"out": False}),
                      ("plane", "three planes", {"hits": 1}), COUNT, WAVELENGTH],
            "fresnel": [("system", "", {"sys": "fresnel"}, {}),
                        ("polarisation", "Polarization must be set", {"in_flags": 0},
                         {"in_flags": _capi.SPOT_POLARIZED_OK})],
        },
        singles=[("no rays", {"n": 0}), ("wavelength -1", {"wl": -1}), ("no hits", {"hits": None}),
                 ("params NULL", {"p": False}), ("inputs NULL", {"in": None})]
        + _refused_systems("forbes", "newton") + _holes("hits", 3),
        accepted=("no rays", "no hits")),
    "ol_trace_spot_batch": dict(
        call=trace_spot_batch,
        valid=dict(sys="plain", dt=F64, n=N, p=True, n_cells=2, cell_wl=1, cell_hy=0.5,
                   optics_of=None, hits=True, stride=N, out=True, in_flags=_capi.RAYGEN_CHECK_FIELD,
                   **{"in": OK}),
        peels={
            "plain": [DTYPE, ("out", "NULL argument", {"out": False}), COUNT,
                      ("cells", "cells outside", {"n_cells": _capi.SPOT_BATCH_MAX_CELLS + 1}),
                      ("field planes", "per-ray field", {"in": "field planes"}),
                      ("stride", "hits_stride", {"stride": N - 1}),
                      ("cell wavelength", "wavelength index", {"cell_wl": 3}),
                      ("cell field", "Normalized field", {"cell_hy": 1.5})],
            "fresnel": [("system", "", {"sys": "fresnel", "cell_wl": 0}, {}),
                        ("polarisation", "Polarization must be set", {},
                         {"in_flags": _capi.RAYGEN_CHECK_FIELD | _capi.SPOT_POLARIZED_OK})],
        },
        singles=[("no rays", {"n": 0}), ("no cells", {"n_cells": 0}), ("cells -1", {"n_cells": -1}),
                 ("cell wavelength -1", {"cell_wl": -1}), ("no hits", {"hits": False}),
                 ("optics of another size", {"optics_of": "other"}),
                 ("optics of itself", {"optics_of": "plain"}), ("params NULL", {"p": False})]
        + _refused_systems("forbes", "newton"),
        accepted=("no rays", "no cells", "no hits", "optics of itself")),
    "ol_trace_opd": dict(
        call=trace_opd,
        valid=dict(sys="plain", dt=F64, n=N, p=True, wl=0, pupil=OK, moments=True, **{"in": OK}),
        peels={"plain": [("dtype", "fp64 only", {"dt": F32}), ("moments", "NULL argument", {"moments": False}),
                         ("plane", "pupil planes", {"pupil": 1}), COUNT, WAVELENGTH,
                         ("field planes", "one field point", {"in": "field planes"})]},
        singles=[("dtype 7", {"dt": 7}), ("no rays", {"n": 0}), ("wavelength -1", {"wl": -1}),
                 ("no pupil", {"pupil": None}), ("params NULL", {"p": False})]
        + _refused_systems("fresnel", "forbes", "newton") + _holes("pupil", 3),
        accepted=("no rays", "no pupil")),
    "ol_wavefront_reference": dict(
        call=wavefront_reference,
        valid=dict(sys="plain", dt=F64, p=True, wl=0, reference=True, **{"in": OK}),
        peels={"plain": [("dtype", "fp64 only", {"dt": F32}), WAVELENGTH,
                         ("reference", "NULL argument", {"reference": False}),
                         ("field planes", "one field point", {"in": "field planes"})]},
        singles=[("dtype 7", {"dt": 7}), ("wavelength -1", {"wl": -1}), ("params NULL", {"p": False}),
                 ("inputs NULL", {"in": None})] + _refused_systems("fresnel", "forbes", "newton"),
        accepted=()),
    "ol_trace_opd_dev": dict(
        call=trace_opd_dev,
        valid=dict(sys="plain", dt=F64, n=N, p=True, wl=0, pupil=OK, moments=True, **{"in": OK}),
        peels={"plain": [("dtype", "fp64 only", {"dt": F32}), WAVELENGTH,
                         ("moments", "NULL argument", {"moments": False}),
                         ("plane", "three planes", {"pupil": 1}), COUNT,
                         ("field planes", "one field point", {"in": "field planes"})]},
        singles=[("dtype 7", {"dt": 7}), ("no rays", {"n": 0}), ("wavelength -1", {"wl": -1}),
                 ("no pupil", {"pupil": None}), ("params NULL", {"p": False})]
        + _refused_systems("fresnel", "forbes", "newton") + _holes("pupil", 3),
        accepted=("no rays", "no pupil")),
}

DEVICE_ENTRIES = {
    "ol_trace_forbes": dict(
        call=trace_forbes,
        valid=dict(sys="forbes", dt=F64, n=N, rays=OK, wl=0, record=True, stride=N, surface=1,
                   flags=0),
        peels={"forbes": [DTYPE, COUNT, ("surface", "surface 4 outside", {"surface": 4}), WAVELENGTH,
                          ("flags", "flags 0x", {"flags": 0x4}), ("plane", "rays[3]", {"rays": 3}),
                          ("stride", "record_stride", {"stride": N - 1})]},
        singles=[("no rays", {"n": 0}), ("surface -1", {"surface": -1}),
                 ("not a forbes surface", {"surface": 2}), ("wavelength -1", {"wl": -1}),
                 ("rays NULL", {"rays": None}), ("nothing to write", {"record": False}),
                 ("write rays alone", {"record": False, "flags": S.TRACE_WRITE_RAYS}),
                 ("coated", {"sys": "forbes_coated"})]
        + _holes("rays", 8),
        accepted=("no rays", "write rays alone")),
    "ol_aim_rays": dict(
        call=aim_rays,
        valid=dict(sys="aim", n=N, wl=0, first=1, stop=9, p=True, guess=None, out=OK, status=True,
                   tol=1e-6, max_iter=10, hy0=0.7, **{"in": OK}),
        peels={"aim": [("params", "params is NULL", {"p": False}), ("pupil", "px, py", {"in": "no py"}),
                       ("status", "status is NULL", {"status": False}), COUNT,
                       ("out plane", "out[3]", {"out": 3}), ("guess plane", "guess[1]", {"guess": 1}),
                       WAVELENGTH, ("range", "surface range", {"first": 10}),
                       ("max_iter", "max_iter", {"max_iter": -1}), ("tol", "tol -1", {"tol": -1.0})]},
        singles=[("no rays", {"n": 0}), ("out NULL", {"out": None}), ("hx alone", {"in": "hx alone"}),
                 ("first -1", {"first": -1}), ("stop past the table", {"stop": 21}),
                 ("wavelength -1", {"wl": -1}), ("inputs NULL", {"in": None}),
                 ("forbes range", {"sys": "forbes", "first": 0, "stop": 3}),
                 ("reference newton range", {"sys": "newton", "first": 1, "stop": 4})]
        + _holes("out", 6) + _holes("guess", 6),
        accepted=("no rays",)),
}

# A range that holds rows of two one-launch kinds answers the kind that is refused first (Forbes,
# then grating, phase, grid sag), not the surface that comes first: [entry, call, arguments].  The
# table has the grating at row 3 and the Forbes row at row 5; the answers of the parent commit are
# the fixture's section "two_kinds".
TWO_KINDS = [
    ["ol_trace", trace, dict(sys="two_kinds", dt=F64, n=N, rays=OK, wl=0, record=True, stride=N,
                             prt=False, first=0, last=5, flags=0)],
    ["ol_trace behind the grating", trace,
     dict(sys="two_kinds", dt=F64, n=N, rays=OK, wl=0, record=True, stride=N, prt=False, first=4,
          last=5, flags=0)],
    ["ol_trace in front of the forbes row", trace,
     dict(sys="two_kinds", dt=F64, n=N, rays=OK, wl=0, record=True, stride=N, prt=False, first=0,
          last=4, flags=0)],
    ["ol_newton_count", newton_count, dict(sys="two_kinds", dt=F64, n=N, rays=OK, wl=0, first=0,
                                           surface=5, iterations=True)],
    ["ol_trace_generate", trace_generate,
     dict(sys="two_kinds", dt=F64, n=N, p=True, wl=0, record=True, stride=N, rays_out=None,
          prt=False, flags=0, extras=None, **{"in": OK})],
]


def two_kinds(k: Context) -> list:
    """[[case, return code, text], ...] of TWO_KINDS."""
    return [[case, *_answer(k, {"call": call}, a)] for case, call, a in TWO_KINDS]


# the current-device rule, recorded and replayed only where two devices are visible
OTHER_DEVICE = "other device current"


# ------------------------------------------------------------------ running them
def _answer(k: Context, entry, a):
    rc = entry["call"](k, a)
    return rc, (OK if rc == 0 else k.lib.ol_last_error().decode("utf-8", "replace"))


def _broken(k: Context, fault, a):
    """The arguments of `fault` on top of `a` (the wavelength fault: n_wl of the call's system)."""
    out = dict(fault[2])
    if fault is WAVELENGTH:
        out["wl"] = int(k.tables[{**a, **out}["sys"]].optics.shape[1])
    return out


def run(k: Context, name: str, entry: dict, order: dict | None = None) -> list:
    """Every case of one entry: [[case, return code, text], ...].  `order`: per peeling sequence the
    fault to repair after each refusal (a replay of the fixture); None: the fault whose piece of
    text the refusal carries (the recorder), each of them exactly once."""
    out = []
    rc, text = _answer(k, entry, {**entry["valid"], "sys": None})
    out.append(["null system", rc, text])
    for label, faults in entry["peels"].items():
        a = dict(entry["valid"])
        for f in faults:
            a.update(_broken(k, f, a))
        left = {f[0]: f for f in faults if f[1]}       # (no text: the choice of the system)
        steps = list(order[label]) if order is not None else None
        while True:
            rc, text = _answer(k, entry, a)
            if order is not None:
                fault = steps.pop(0) if steps else None
            else:
                hit = [n for n, f in left.items() if f[1] in text] if rc else []
                assert rc == 0 or len(hit) == 1, (name, label, rc, text, sorted(left))
                fault = hit[0] if rc else None
            out.append([f"{label}: {fault or 'accepted'}", rc, text])
            if fault is None:
                break
            f = left.pop(fault)
            a.update(f[3] if len(f) > 3 else {key: entry["valid"][key] for key in f[2]})
        if order is None:
            assert not left, f"{name} / {label}: accepted with {sorted(left)} never reported"
    for label, change in entry["singles"]:
        rc, text = _answer(k, entry, {**entry["valid"], **change})
        out.append([label, rc, text])
    return out


def peel_order(cases: list) -> dict:
    """label -> the faults a recorded peeling sequence repaired, in order."""
    out = {}
    for case, _rc, _text in cases:
        if ": " in case:
            label, fault = case.split(": ", 1)
            out.setdefault(label, [])
            if fault != "accepted":
                out[label].append(fault)
    return out


def other_device(k: Context) -> list:
    """ol_trace_ex on a system of device 0 while device 1 is current."""
    import torch

    with torch.cuda.device(1):
        rc, text = _answer(k, ENTRIES["ol_trace_ex"], ENTRIES["ol_trace_ex"]["valid"])
    return [OTHER_DEVICE, rc, text]


def replay(k: Context, section: dict, entries: dict, report=print) -> int:
    """Replays one section of the fixture: every case's code and text equal to the recorded ones,
    every peeling sequence ends accepted.  Returns the number of cases compared."""
    assert sorted(section) == sorted(entries), (sorted(section), sorted(entries))
    count, bad = 0, []
    for name, entry in entries.items():
        want = [c for c in section[name] if c[0] != OTHER_DEVICE]
        got = run(k, name, entry, peel_order(want))
        assert [c[0] for c in got] == [c[0] for c in want], (name, "the cases themselves differ")
        for g, w in zip(got, want):
            count += 1
            if g != w:
                bad.append(f"{name} / {w[0]}: got {g[1]} {g[2]!r}, recorded {w[1]} {w[2]!r}")
        for label in entry["peels"]:
            assert [f"{label}: accepted", 0, OK] in got, (name, label, "does not end accepted")
    report(f"{count} cases replayed, {len(bad)} differ")
    assert not bad, "\n".join(bad)
    return count


# ------------------------------------------------------------------ ol_system_create / _update
# What STAGING refuses (the host-side conversion of a table, before any device call): single-fault
# calls -- staging returns at the first fault, so nothing peels -- each next to the accepted
# neighbour where one exists.  A case: (name, accepted, table, row, fields of that row to set,
# edits of the call).  Edits: "coeffs" {index: value}, "buffer" (a new coefficient buffer), and the
# arguments themselves: "surf" / "buffer_ptr" / "optics" None for a NULL pointer, "n_surf",
# "n_coeffs", "n_wl".  Fields: "aperture[1]" sets one element.  The block rules of the four
# one-launch kinds are pinned by their own tests (tests/test_*_cpu.py), not here.
def _golden(name: str) -> SystemTable:
    return SystemTable.load(os.path.join(HERE, "golden", f"{name}.json"))


def create_tables() -> dict:
    """plain: no coefficients, 3 wavelengths.  boolean: token lists at [0, 35) and [35, 60) of 60.
    zernike: 12 terms at [0, 48) of 48.  f3: biconic (row 1), toroidal (2, 5), Chebyshev (row 3:
    9 values, 3 columns, at [6, 17) of 21).  retarder: the axis block [0, 4) of 4, row 2."""
    return {"plain": load_system("double_gauss"), "boolean": _golden("boolean_apertures"),
            "zernike": load_system("zernike_fresnel_fringe"), "f3": _golden("f3_family"),
            "asphere": load_system("rc_asphere"), "retarder": retarder_table()}


def _tree(leaves: int, polygon_at: int | None = None) -> list:
    """`leaves` radial leaves, then the unions that join them: a tree of depth `leaves`.  One leaf
    may be a polygon of two vertices (its vertex block: the first four values of the buffer)."""
    toks = [[S.AP_RADIAL, 0.0, 5.0, 0.0, 0.0] for _ in range(leaves)]
    if polygon_at is not None:
        toks[polygon_at] = [S.AP_POLYGON, 0.0, 2.0, 0.0, 0.0]
    toks += [[S.AP_OP_UNION, 0.0, 0.0, 0.0, 0.0]] * (leaves - 1)
    return [v for t in toks for v in t]


def _composite(tokens: list, count: int | None = None):
    """Row 3 of the plain lens with `tokens` as its aperture."""
    count = len(tokens) // 5 if count is None else count
    return ("plain", 3, {"aperture_kind": S.AP_COMPOSITE, "aperture[0]": 0.0,
                         "aperture[1]": float(count)}, {"buffer": tokens})


_SQUARE = [-5.0, -5.0, 5.0, -5.0, 5.0, 5.0, -5.0, 5.0]
_LEAF, _UNION = _tree(1), [S.AP_OP_UNION, 0.0, 0.0, 0.0, 0.0]


def _polygon(voff, nv):
    return ("plain", 3, {"aperture_kind": S.AP_POLYGON, "aperture[0]": voff, "aperture[1]": nv},
            {"buffer": _SQUARE})


def _polygon_token(voff, nv):   # the first leaf of the boolean table's first list
    return ("boolean", None, {}, {"coeffs": {0: S.AP_POLYGON, 1: voff, 2: nv}})


def _zernike_term(n, m):        # the first term of the Zernike row: (c, n, m, N)
    return ("zernike", None, {}, {"coeffs": {0: 1.0, 1: n, 2: m}})


CREATE = [
    ("plain", True, "plain", None, {}, {}),
    ("surfaces NULL", False, "plain", None, {}, {"surf": None}),
    ("no surfaces", False, "plain", None, {}, {"n_surf": 0}),
    ("optics NULL", False, "plain", None, {}, {"optics": None}),
    ("no wavelengths", False, "plain", None, {}, {"n_wl": 0}),
    ("negative coefficient count", False, "plain", None, {}, {"n_coeffs": -1}),
    ("coefficients NULL with a count", False, "zernike", None, {}, {"buffer_ptr": None}),
    # the kinds: below and above their ranges, the two numbers no kind has
    ("geometry -1", False, "plain", 3, {"geom_kind": -1}, {}),
    ("geometry 0", True, "plain", 3, {"geom_kind": S.GEOM_PLANE}, {}),
    ("geometry 13", False, "plain", 3, {"geom_kind": 13}, {}),
    ("geometry 15", False, "plain", 3, {"geom_kind": 15}, {}),
    ("geometry 17", False, "plain", 3, {"geom_kind": 17}, {}),
    ("interaction -1", False, "plain", 3, {"interaction": -1}, {}),
    ("interaction 2", True, "plain", 3, {"interaction": S.INTERACT_REFLECT}, {}),
    ("interaction 3", False, "plain", 3, {"interaction": 3}, {}),
    ("aperture kind -1", False, "plain", 3, {"aperture_kind": -1}, {}),
    ("aperture kind 7", False, "plain", 3, {"aperture_kind": 7}, {}),
    ("coating kind -1", False, "plain", 3, {"coating_kind": -1}, {}),
    ("coating kind 2", True, "plain", 3, {"coating_kind": S.COAT_FRESNEL}, {}),
    ("coating kind 5", False, "plain", 3, {"coating_kind": 5}, {}),
    ("negative n_coeff", False, "plain", 3, {"n_coeff": -1}, {}),
    ("negative coeff_offset", False, "plain", 3, {"coeff_offset": -1}, {}),
    # a coefficient block against the end of the buffer: four values per Zernike term, two in front
    # of a Chebyshev grid, one per value otherwise
    ("zernike block fits exactly", True, "zernike", None, {}, {}),
    ("zernike block one value short", False, "zernike", None, {}, {"n_coeffs": 47}),
    ("zernike block one term too many", False, "zernike", 1, {"n_coeff": 13}, {}),
    ("chebyshev block fits exactly", True, "f3", 3, {"coeff_offset": 10}, {}),
    ("chebyshev block one value too many", False, "f3", 3, {"coeff_offset": 11}, {}),
    ("toroidal block fits exactly", True, "f3", None, {}, {}),
    ("toroidal block one value too many", False, "f3", 5, {"coeff_offset": 20}, {}),
    ("asphere", True, "asphere", None, {}, {}),
    # polygon vertex blocks: a top-level aperture, a leaf of a token list
    ("polygon fits exactly", True, *_polygon(0.0, 4.0)),
    ("polygon one vertex too many", False, *_polygon(0.0, 5.0)),
    ("polygon shifted by one value", False, *_polygon(1.0, 4.0)),
    ("polygon offset -1", False, *_polygon(-1.0, 4.0)),
    ("polygon without a vertex", False, *_polygon(0.0, 0.0)),
    ("polygon of one vertex", True, *_polygon(0.0, 1.0)),
    ("polygon leaf fits exactly", True, *_polygon_token(40.0, 10.0)),
    ("polygon leaf one vertex too many", False, *_polygon_token(40.0, 11.0)),
    ("polygon leaf without a vertex", False, *_polygon_token(40.0, 0.0)),
    # aperture token lists
    ("token lists fit exactly", True, "boolean", None, {}, {}),
    ("token list one token too many", False, "boolean", 2, {"aperture[1]": 6.0}, {}),
    ("token list of no tokens", False, "boolean", 2, {"aperture[1]": 0.0}, {}),
    ("token list offset -1", False, "boolean", 2, {"aperture[0]": -1.0}, {}),
    ("tree of depth 16", True, *_composite(_tree(16))),
    ("tree of depth 17", False, *_composite(_tree(17))),
    ("tree of depth 16, the last leaf a polygon", True, *_composite(_tree(16, polygon_at=15))),
    ("tree of depth 17, the last leaf a polygon", False, *_composite(_tree(17, polygon_at=16))),
    ("one leaf", True, *_composite(_LEAF)),
    ("two leaves and an operator", True, *_composite(_tree(2))),
    ("an operator first", False, *_composite(_UNION)),
    ("an operator behind one leaf", False, *_composite(_LEAF + _UNION)),
    ("two leaves and no operator", False, *_composite(_LEAF + _LEAF)),
    ("token op 0", False, *_composite([0.0] * 5)),
    ("token op 9", False, *_composite([9.0] + [0.0] * 4)),
    ("token op 13", False, *_composite(_tree(2)[:10] + [13.0] + [0.0] * 4)),
    # coating axis blocks: three values for a polarizer, four for a retarder
    ("retarder block fits exactly", True, "retarder", None, {}, {}),
    ("retarder block one value too many", False, "retarder", 2, {"coat[0]": 1.0}, {}),
    ("retarder block offset -1", False, "retarder", 2, {"coat[0]": -1.0}, {}),
    ("polarizer block fits exactly", True, "retarder", 2,
     {"coating_kind": S.COAT_POLARIZER, "coat[0]": 1.0}, {}),
    ("polarizer block one value too many", False, "retarder", 2,
     {"coating_kind": S.COAT_POLARIZER, "coat[0]": 2.0}, {}),
    # Zernike indices
    ("zernike n 60", True, *_zernike_term(60.0, 0.0)),
    ("zernike n 62", False, *_zernike_term(62.0, 0.0)),
    ("zernike n below |m|", False, *_zernike_term(1.0, -3.0)),
    ("zernike n - |m| odd", False, *_zernike_term(3.0, 0.0)),
    ("zernike bad index on a term that is zero", True, "zernike", None, {},
     {"coeffs": {0: 0.0, 1: 3.0, 2: 0.0}}),
    # coefficient grids
    ("chebyshev of one row", True, "f3", 3, {"poly_cols": 9}, {}),
    ("chebyshev without columns", False, "f3", 3, {"poly_cols": 0}, {}),
    ("chebyshev ragged", False, "f3", 3, {"poly_cols": 2}, {}),
    ("polynomial", True, "f3", 3, {"geom_kind": S.GEOM_POLYNOMIAL}, {}),
    ("polynomial without columns", False, "f3", 3,
     {"geom_kind": S.GEOM_POLYNOMIAL, "poly_cols": 0}, {}),
    ("polynomial ragged", False, "f3", 3, {"geom_kind": S.GEOM_POLYNOMIAL, "poly_cols": 2}, {}),
    # blocks of a fixed shape
    ("biconic of one value", False, "f3", 1, {"n_coeff": 1}, {}),
    ("biconic of three values", False, "f3", 1, {"n_coeff": 3}, {}),
    ("toroidal of one value", False, "f3", 5, {"n_coeff": 1}, {}),
    ("toroidal without a block", False, "f3", 5, {"n_coeff": 0}, {}),
]

# ol_system_update on a system made from the f3 table (7 rows, one wavelength; its device block has
# room for 64 values more): (name, accepted, system given, table, row, fields, edits).  The last
# toroidal row (2 values at 19) is moved to the end of a longer buffer to grow it.
_LONG = [0.0] * 21 + [50.0, 0.0] + [0.0] * 65


def _grown(terms):
    return ("f3", 5, {"coeff_offset": 21, "n_coeff": 2 + terms}, {"buffer": _LONG})


UPDATE = [
    ("system NULL", False, False, "f3", None, {}, {}),
    ("unchanged", True, True, "f3", None, {}, {}),
    ("one surface fewer", False, True, "f3", None, {}, {"n_surf": 6}),
    ("one wavelength more", False, True, "f3", None, {}, {"n_wl": 2}),
    ("surfaces NULL", False, True, "f3", None, {}, {"surf": None}),
    ("biconic of three values", False, True, "f3", 1, {"n_coeff": 3}, {}),
    ("block grown by 65 values", False, True, *_grown(65)),
    ("block grown by 64 values", True, True, *_grown(64)),
]


def _edited(base: SystemTable, row, fields: dict, edits: dict) -> SystemTable:
    t = _copy(base)
    t.coeffs = np.array(edits.get("buffer", t.coeffs), dtype=np.float64)
    for i, v in edits.get("coeffs", {}).items():
        t.coeffs[i] = v
    for key, v in fields.items():
        name, _, index = key.partition("[")
        if index:
            t.surfaces[name][row][int(index[:-1])] = v
        else:
            t.surfaces[name][row] = v
    return t


def _table_args(t: SystemTable, edits: dict):
    """(what keeps the arrays alive, the six table arguments of ol_system_create / _update)."""
    surf, optics = np.ascontiguousarray(t.surfaces), np.ascontiguousarray(t.optics)
    coeffs = np.ascontiguousarray(t.coeffs, dtype=np.float64)
    a = {"surf": OK, "n_surf": surf.shape[0], "buffer_ptr": OK if coeffs.size else None,
         "n_coeffs": coeffs.size, "optics": OK, "n_wl": optics.shape[1], **edits}
    return (surf, optics, coeffs), (
        surf.ctypes.data if a["surf"] else None, a["n_surf"],
        coeffs.ctypes.data if a["buffer_ptr"] else None, a["n_coeffs"],
        optics.ctypes.data if a["optics"] else None, a["n_wl"])


def create(lib) -> list:
    """[[case, return code, text], ...] of CREATE and UPDATE ("update: ..."); every system an
    accepted call made is destroyed."""
    base, out = create_tables(), []

    def answer(rc):
        return rc, (OK if rc == 0 else lib.ol_last_error().decode("utf-8", "replace"))

    for case, _accepted, name, row, fields, edits in CREATE:
        keep, args = _table_args(_edited(base[name], row, fields, edits), edits)
        h = C.c_void_p()
        out.append([case, *answer(lib.ol_system_create(*args, C.byref(h)))])
        assert bool(h) == (out[-1][1] == 0), case
        lib.ol_system_destroy(h)
    keep, args = _table_args(base["f3"], {})
    system = C.c_void_p()
    assert lib.ol_system_create(*args, C.byref(system)) == 0, lib.ol_last_error()
    for case, _accepted, given, name, row, fields, edits in UPDATE:
        keep, args = _table_args(_edited(base[name], row, fields, edits), edits)
        out.append([f"update: {case}",
                    *answer(lib.ol_system_update(system if given else None, *args, None))])
    lib.ol_system_destroy(system)
    return out


def create_accepted() -> list:
    """The case names of create() with whether each is meant to be accepted."""
    return [(c[0], c[1]) for c in CREATE] + [(f"update: {c[0]}", c[1]) for c in UPDATE]
