"""Modulation transfer functions on the device, stand-alone (no reference package needed).

`GeometricMTF` mirrors the reference's class of that name (optiland/mtf/geometric.py:27-204):
the image-plane hits of every field come from ONE batched spot launch (`ol_trace_spot_batch`),
and every field's tangential (y) and sagittal (x) curve from ONE `ol_geometric_mtf` call --
three kernels for the histogram and the transform of all curves instead of the reference's
Python loop over the frequencies.  The numbers are those of the reference's NumPy backend
(fp64 `np.histogram`), not of its torch backend, which bins in float32.

`FFTMTF` mirrors `ScalarFFTMTF` (optiland/mtf/fft.py:19-235) on top of `wavefront.FFTPSF` and
`torch.fft`; no kernel of its own.

`SampledMTF` mirrors the reference's fast MTF (optiland/mtf/sampled.py:17-207): the fused OPD map,
its Zernike fit (`ol_zernike_fit`) and the overlap sums of ALL requested frequencies in one
`ol_sampled_mtf` call instead of a Python loop that re-evaluates the basis per frequency.
"""

from __future__ import annotations

import numpy as np
import torch

from .wavefront import FFTPSF, Wavefront, calculate_grid_size, working_fno


def _resolve_fields(table, fields):
    """utils.resolve_fields: 'all' = the optic's fields, normalised by the largest."""
    if isinstance(fields, str):
        if fields != "all":
            raise ValueError("Invalid fields string. Must be 'all' or a list of coordinates.")
        mf = table.raygen.get("max_field", 0.0) or 1.0
        fields = [(f[0] / mf, f[1] / mf) for f in table.fields]
    return [(float(f[0]), float(f[1])) for f in fields]


def _resolve_wavelength(table, wavelength) -> float:
    """utils.py:229-253 resolve_wavelength."""
    if isinstance(wavelength, str):
        if wavelength != "primary":
            raise ValueError("Invalid wavelength string. For a single wavelength, it must be "
                             "'primary'.")
        if table.primary_wavelength is not None:
            return float(table.primary_wavelength)
        return float(table.wavelengths[table.reference_wavelength_index()])
    if isinstance(wavelength, bool) or not isinstance(wavelength, (int, float)):
        if hasattr(wavelength, "item"):
            return float(wavelength.item())
        raise TypeError("Wavelength must be a string ('primary') or a number.")
    return float(wavelength)


def paraxial_fno(table) -> float:
    """`optic.paraxial.FNO()` (paraxial.py:277-289) from the packed table: f2 / EPD, f2 from the
    reference's y-u trace of a ray parallel to the axis at the primary wavelength
    (paraxial.py:74-86, restated in paraxial_host).  (An image-space F/# aperture answers with
    its own value in the reference; its EPD is f2 / value, so the quotient is that value to
    within a rounding.)"""
    from . import paraxial_host
    from . import system as S

    surf = table.surfaces
    wi = table.reference_wavelength_index()
    n = [float(v) for v in table.optics[:, wi]["n2"]]
    pos = [float(v) for v in surf["origin"][:, 2]]
    reflect = (surf["interaction"] == S.INTERACT_REFLECT).tolist()
    radii = [float(r) for r in surf["radius"]]
    y, u = paraxial_host._trace(radii, n, pos, reflect, 1.0, 0.0, pos[1] - 1.0)
    epd = float(table.raygen["EPD"])
    if u[-1] == 0.0 or epd == 0.0:
        raise ValueError("paraxial F/# undefined (afocal system or zero entrance pupil)")
    return (-y[0] / u[-1]) / epd


def diffraction_limited_scale(freq: np.ndarray, cutoff_freq: float) -> np.ndarray:
    """geometric.py:160-163: the MTF of an aberration-free circular pupil."""
    ratio = np.clip(np.asarray(freq, dtype=np.float64) / cutoff_freq, 0.0, 1.0)
    phi = np.arccos(ratio)
    return 2 / np.pi * (phi - np.cos(phi) * np.sin(phi))


class GeometricMTF:
    """Geometric MTF (mtf/geometric.py:27-204; Smith, Modern Optical Engineering, 3rd ed.,
    section 11.9) of `tracer`'s system, same arguments and attributes as the reference:
    `freq` (num_points,), `mtf[field] = [tangential, sagittal]` (float64 device tensors; the
    tangential curve is the one of the hits' y, the sagittal the one of their x),
    `diff_limited_mtf` (the scale factor, or 1 with `scale=False`), `max_freq`, `cutoff_freq`.
    `mtf_all` holds the (fields, 2, num_points) block the lists are views of."""

    def __init__(self, tracer, fields="all", wavelength="primary", num_rays: int = 100,
                 distribution: str = "uniform", num_points: int = 256, max_freq="cutoff",
                 scale: bool = True):
        table = tracer.table
        self.tracer = tracer
        self.num_points, self.scale = int(num_points), scale
        self.num_rays, self.distribution = num_rays, distribution
        self.wavelength = _resolve_wavelength(table, wavelength)
        # wavelength in mm for a frequency in cycles / mm (geometric.py:84-90)
        self.cutoff_freq = 1 / (self.wavelength * 1e-3 * paraxial_fno(table))
        self.max_freq = self.cutoff_freq if isinstance(max_freq, str) and max_freq == "cutoff" \
            else max_freq
        self.fields = _resolve_fields(table, fields)
        self.freq = np.linspace(0, self.max_freq, self.num_points)
        self.data = self._hits()
        self.mtf, self.diff_limited_mtf = self._generate_mtf_data()

    def _hits(self):
        """[(x, y) per field]: the image-plane hits with intensity > 0 in the image surface's
        frame (analysis/spot_diagram/core.py:440-481), all fields in one launch."""
        t, eng = self.tracer, self.tracer.engine
        s = t.table.surfaces[-1]
        if s["flags"] & 1:
            raise NotImplementedError("geometric MTF on a tilted image surface")
        ox, oy = float(s["origin"][0]), float(s["origin"][1])
        if hasattr(eng, "trace_spot_batch"):
            px, py = t._pupil_planes(self.distribution, self.num_rays)
            n = int(px.numel())
            wl, _ = t._wavelength_index(self.wavelength)
            cells = []
            for hx, hy in self.fields:
                t._validate_normalized_coordinates(hx, hy, "field")
                vx, vy = t._vig_scalar(hx, hy)
                cells.append((hx, hy, vx, vy, 0.0, 0.0, wl))
            _mom, hb = eng.trace_spot_batch(px, py, cells, hits=True)
            planes = [(hb[k, 0, :n], hb[k, 1, :n], hb[k, 2, :n]) for k in range(len(cells))]
        else:   # (engines without the batch entry point: one fused spot launch per field)
            planes = [t.trace_spot(hx, hy, self.wavelength, self.num_rays, self.distribution,
                                   hits=True)[1] for hx, hy in self.fields]
        alive = [p[2] > 0 for p in planes]
        # (one read-back: is any ray of any field vignetted or lost?)
        clipped = not bool(torch.stack([a.all() for a in alive]).all()) if alive else False
        out = []
        for (x, y, _i), keep in zip(planes, alive):
            if clipped:
                x, y = x[keep], y[keep]
            out.append((x - ox if ox != 0.0 else x, y - oy if oy != 0.0 else y))
        return out

    def _transform(self, curves, scale):
        """(curves, num_points) float64: `ol_geometric_mtf` on the tracer's device."""
        from .engine import geometric_mtf
        return geometric_mtf(curves, self.freq, scale, self.num_points + 1,
                             device=self.tracer.device)

    def _generate_mtf_data(self):
        """geometric.py:152-177."""
        scale = diffraction_limited_scale(self.freq, self.cutoff_freq) if self.scale else None
        curves = [c for x, y in self.data for c in (y, x)]   # [tangential, sagittal] per field
        self.mtf_all = self._transform(curves, scale).reshape(len(self.data), 2, self.num_points)
        mtf = [[m[0], m[1]] for m in self.mtf_all]
        return mtf, (scale if scale is not None else 1)


class FFTMTF:
    """Scalar FFT MTF (mtf/fft.py:19-235 `ScalarFFTMTF`): per field the FFT PSF of
    `wavefront.FFTPSF`, |fft2|, the tangential and the sagittal slice from the DC bin outward,
    normalised by the DC value and clipped to [0, 1].  `mtf[field] = [tangential, sagittal]`
    (device tensors of grid_size // 2 entries), `freq_tang[field]` / `freq_sag[field]` the
    two frequency axes in cycles / mm (`freq` = `freq_tang`), `FNO[field]` the working F/#.
    Scalar only: a polarised system is the reference's `VectorialFFTMTF`, not built here."""

    def __init__(self, tracer, fields="all", wavelength="primary", num_rays: int = 128,
                 grid_size=None, max_freq="cutoff", strategy: str = "chief_ray",
                 remove_tilt: bool = False, **kwargs):
        table = tracer.table
        if table.polarization is not None:
            raise NotImplementedError("FFTMTF: polarised system -- the reference answers with "
                                      "VectorialFFTMTF, which is not built here")
        if grid_size is None:
            self.num_rays, self.grid_size = calculate_grid_size(num_rays)
        else:
            self.num_rays, self.grid_size = num_rays, grid_size
        self.tracer = tracer
        self.resolved_fields = _resolve_fields(table, fields)
        self.resolved_wavelength = _resolve_wavelength(table, wavelength)
        self.psf = [FFTPSF(tracer, f, self.resolved_wavelength, self.num_rays, self.grid_size,
                           strategy, remove_tilt, **kwargs).psf for f in self.resolved_fields]
        self.mtf = self._generate_mtf_data()
        w = self.resolved_wavelength
        self.FNO = [working_fno(tracer, f, w) for f in self.resolved_fields]
        self._on_axis_fno = working_fno(tracer, (0.0, 0.0), w)
        self.max_freq = 1 / (w * 1e-3 * self._on_axis_fno) \
            if isinstance(max_freq, str) and max_freq == "cutoff" else max_freq
        k = np.arange(self.grid_size // 2)
        self.freq_tang = [k * self._units_tang(i) for i in range(len(self.FNO))]
        self.freq_sag = [k * self._units_sag(i) for i in range(len(self.FNO))]
        self.freq = self.freq_tang

    def _generate_mtf_data(self):
        """fft.py:156-194."""
        c = self.grid_size // 2
        mtf = []
        for psf in self.psf:
            data = torch.abs(torch.fft.fftshift(torch.fft.fft2(psf)))
            tang, sag, dc = data[c:, c][:c], data[c, c:][:c], data[c, c]
            if float(dc) == 0:
                tang, sag = torch.zeros_like(tang), torch.zeros_like(sag)
            else:
                tang, sag = tang / dc, sag / dc
            mtf.append([torch.clip(tang, 0.0, 1.0), torch.clip(sag, 0.0, 1.0)])
        return mtf

    def _units_sag(self, k) -> float:
        """fft.py:220-235."""
        return 1 / ((self.num_rays - 1) * self.resolved_wavelength * 1e-3 * self.FNO[k])

    def _units_tang(self, k) -> float:
        """fft.py:196-218: the chief ray's tilt compresses the tangential axis."""
        return self._units_sag(k) * (self._on_axis_fno / self.FNO[k])


def paraxial_exit_pupil(table):
    """(XPD, XPL) of `optic.paraxial` (paraxial.py:244-275) from the packed table: XPL is the
    exit-pupil position the table carries, relative to the image surface; XPD twice the height
    of the paraxial marginal ray (paraxial.py:316-345, restated in paraxial_host) there."""
    from . import paraxial_host
    from . import system as S

    surf, rg = table.surfaces, table.raygen
    wi = table.reference_wavelength_index()
    n = [float(v) for v in table.optics[:, wi]["n2"]]
    pos = [float(v) for v in surf["origin"][:, 2]]
    reflect = (surf["interaction"] == S.INTERACT_REFLECT).tolist()
    radii = [float(r) for r in surf["radius"]]
    xpl = float(rg["pupil_z"]) - pos[-1]
    epd = float(rg["EPD"])
    if rg.get("object_infinite"):
        ya, ua, z0 = epd / 2, 0.0, pos[1] - 10.0
    else:
        z0 = pos[0]
        ya, ua = 0.0, epd / (2 * (float(rg["EPL"]) - z0))
    y, u = paraxial_host._trace(radii, n, pos, reflect, ya, ua, z0)
    return 2 * (y[-1] + u[-1] * xpl), xpl


def pupil_shifts(frequencies, wavelength_um: float, xpd: float, xpl: float) -> np.ndarray:
    """sampled.py:158-178: the (F, 2) pupil shifts, in normalised pupil units, of spatial
    frequencies (fx, fy) in cycles / mm; `xpl` is the class's attribute (minus the paraxial
    XPL).  The operations and their order are the reference's."""
    wl_mm = wavelength_um * 1e-3
    f = np.asarray(frequencies, dtype=np.float64).reshape(-1, 2)
    return xpl * (wl_mm * f) / (xpd / 2)


class SampledMTF:
    """The sampled MTF (mtf/sampled.py:17-207) of one field and wavelength: same arguments and
    attributes as the reference -- `x_norm`, `y_norm`, `opd_waves`, `intensity` (float64 device
    tensors), `xpd`, `xpl`, `zernike_coeffs` (the fit of the OPD map over every sample, as
    sampled.py:97-103 fits it), `otf_at_zero`.  `calculate_mtf(frequencies)` returns a list
    with one entry per (fx, fy) pair in cycles / mm: views of ONE device tensor, `mtf_all`."""

    def __init__(self, tracer, field, wavelength, num_rays: int = 128,
                 distribution: str = "uniform", zernike_terms: int = 37,
                 zernike_type: str = "fringe"):
        from . import zernike as Z

        self.zernike_terms = Z.check_terms(zernike_type, zernike_terms, "SampledMTF")
        self.zernike_type = zernike_type
        self.tracer, self.field = tracer, field
        self.wavelength = _resolve_wavelength(tracer.table, wavelength)
        self.num_rays, self.distribution = num_rays, distribution
        wf = Wavefront(tracer, field, self.wavelength, num_rays=num_rays,
                       distribution=distribution)
        self.x_norm, self.y_norm = tracer._dev(wf.distribution.x), tracer._dev(wf.distribution.y)
        self.opd_waves, self.intensity = wf.data.opd, wf.data.intensity
        xpd, xpl = paraxial_exit_pupil(tracer.table)
        self.xpd, self.xpl = xpd, -xpl
        self.zernike_coeffs, status = self._fit()
        if status:
            raise ValueError(f"SampledMTF: {Z.status_text(status)}")
        self.otf_at_zero = self.intensity.sum()

    def _fit(self):
        from .engine import zernike_fit

        c, status = zernike_fit(self.x_norm, self.y_norm, self.opd_waves, self.zernike_type,
                                self.zernike_terms, device=self.tracer.device)
        return c, int(status)

    def _sum(self, shifts):
        from .engine import sampled_mtf

        return sampled_mtf(self.zernike_coeffs, self.zernike_type, self.x_norm, self.y_norm,
                           self.opd_waves, self.intensity, shifts, device=self.tracer.device)

    def calculate_mtf(self, frequencies):
        """sampled.py:108-207."""
        freq = [(float(fx), float(fy)) for fx, fy in frequencies]
        if self.xpd == 0.0:   # sampled.py:163-168
            return [1.0 if fx == 0.0 and fy == 0.0 else 0.0 for fx, fy in freq]
        if not freq:
            return []
        self.mtf_all = self._sum(pupil_shifts(freq, self.wavelength, self.xpd, self.xpl))
        return list(self.mtf_all)
