"""Wavefront OPD and scalar FFT PSF on device.

Mirrors the numerics of the reference's chief-ray wavefront strategy
(optiland/wavefront/strategy.py:142-243), `Wavefront` / `OPD`
(wavefront/wavefront.py:28-176, wavefront/opd.py:145-159) and the scalar FFT PSF
(psf/fft.py:42-262, psf/base.py:418-438):

    chief ray -> reference sphere (centre = chief-ray image point, radius to the
    paraxial exit pupil) -> per-ray OPD in waves (`ol_wavefront_opd`) ->
    pupil function A exp(-i 2 pi OPD) on a uniform grid -> zero-pad -> FFT -> |.|^2.

The trace runs in fp64 (an OPD good to lambda/1000 over a 200 mm path needs 1e-9
relative); the FFT is torch.fft on the ROCm device (rocFFT) -- a plain library
transform, as MFMA GEMMs would be hipBLASLt's job.
"""

from __future__ import annotations

import math

from . import _capi

import numpy as np
import torch

from .distribution import create_distribution


class WavefrontData:
    """wavefront/wavefront_data.py:10-38 (+ the device-side sums of the fused kernel)."""

    def __init__(self, pupil_x, pupil_y, pupil_z, opd, intensity, radius, moments=None):
        self.pupil_x, self.pupil_y, self.pupil_z = pupil_x, pupil_y, pupil_z
        self.opd, self.intensity, self.radius = opd, intensity, radius
        # `ol_trace_opd`'s 12 sums (tilt-fit moments; count / sum / sum of squares of the OPD
        # over rays with i > 0) of the OPD as first computed -- None on the un-fused path.
        # They describe `_moments_of` (that exact tensor) only: consumers check identity, so a
        # caller who replaces or detrends `opd` gets sums recomputed from the data it passes
        self.moments = moments
        self._moments_of = opd if moments is not None else None


class Wavefront:
    """OPD map for ONE field and wavelength (chief-ray strategy, spherical reference)."""

    def __init__(self, tracer, field, wavelength, num_rays: int = 12,
                 distribution="hexapolar", strategy: str = "chief_ray",
                 remove_tilt: bool = False, robust_trim_std: float = 3.0, afocal: bool = False,
                 fused: bool | None = None):
        # wavefront/strategy.py:606-616 (incl. the backward-compatible aliases)
        strategy = {"centroid_sphere": "centroid", "best_fit_sphere": "best_fit"}.get(strategy,
                                                                                       strategy)
        if strategy not in ("chief_ray", "centroid", "best_fit"):
            raise ValueError(f"Unknown wavefront strategy: {strategy}")
        self.strategy = strategy
        self.robust_trim_std = float(robust_trim_std)
        self.remove_tilt = bool(remove_tilt)
        # wavefront.py:74: afocal systems measure against a PLANE (reference_geometry.py:87-128)
        self.afocal = bool(afocal)
        if tracer.dtype != torch.float64:
            raise ValueError("wavefront analysis needs an fp64 tracer (OPD in waves)")
        rg = tracer.table.raygen
        if "pupil_z" not in rg or "n_image" not in rg:
            raise ValueError("this SystemTable carries no exit-pupil data")
        self.tracer = tracer
        # fused generate -> trace -> OPD kernel (`ol_trace_opd`): chief-ray strategy on an
        # unpolarised system; None = use it whenever it applies
        can_fuse = (strategy == "chief_ray" and tracer.table.polarization is None
                    and not tracer.table.uses_polarization
                    and hasattr(tracer.engine, "trace_opd"))
        if fused and not can_fuse:
            raise ValueError("fused OPD needs the chief-ray strategy on an unpolarised system")
        self.fused = can_fuse if fused is None else bool(fused)
        self.field = (float(field[0]), float(field[1]))
        self.wavelength = float(wavelength)
        self.num_rays = num_rays
        if isinstance(distribution, str):
            distribution = create_distribution(distribution)
            distribution.generate_points(num_rays)
        self.distribution = distribution
        self.data = self._compute()
        if self.remove_tilt:  # wavefront.py:173-174
            self.data.opd = self.fit_and_remove_tilt(self.data)
            # the device sums describe the OPD as the kernel produced it, not the detrended
            # map now stored: a later fit (or rms) must take its sums from the data it is
            # given, as the reference's always does
            self.data.moments = None

    @staticmethod
    def fit_and_remove_tilt(data, remove_piston: bool = False, ridge: float = 1e-12):
        """Weighted plane fit of the OPD over the pupil, subtracted (wavefront.py:103-148;
        the piston only with `remove_piston`).  Formulated as what it is on a device: the
        nine weighted moments
            S = sum w [1, x, y, xx, xy, yy],   T = sum w opd [1, x, y]
        -- straight out of the fused kernel's epilogue (`data.moments`), or one (9, n) x (n,)
        reduction on the un-fused path -- the symmetric 3x3 normal system (+ ridge on the
        diagonal, as the reference regularises) solved on the host in closed form, and one
        elementwise pass for the residual."""
        x, y, w, opd = data.pupil_x, data.pupil_y, data.intensity, data.opd
        mom = getattr(data, "moments", None)
        if mom is not None and getattr(data, "_moments_of", None) is opd:
            # the kernel's own sums -- valid only for the very OPD tensor they were taken of
            m = mom[:9].double().cpu().numpy()
        else:
            basis = torch.stack([torch.ones_like(x), x, y, x * x, x * y, y * y,
                                 opd, opd * x, opd * y])
            m = (basis @ w.to(basis.dtype)).double().cpu().numpy()   # one read-back
        A = np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]]) \
            + ridge * np.eye(3)
        a0, bx, cy = np.linalg.solve(A, m[6:9])
        if not remove_piston:
            a0 = 0.0
        return opd - (float(a0) + float(bx) * x + float(cy) * y)

    # strategy.py:83-139: tilt of the launch plane for angle fields at infinity
    def _tilt_cosines(self):
        rg = self.tracer.table.raygen
        # only AngleField at infinity is corrected (strategy.py:113-117); other field
        # types keep their launch-plane tilt, as in the reference
        if not rg.get("object_infinite") or int(rg.get("field_kind", 0)) != 0:
            return 0.0, 0.0
        fx = self.field[0] * rg["max_field"]
        fy = self.field[1] * rg["max_field"]
        tx, ty = math.tan(math.radians(fx)), math.tan(math.radians(fy))
        uz = 1.0 / math.sqrt(1.0 + tx * tx + ty * ty)
        return tx * uz, ty * uz

    def chief_reference(self):
        """(params, R, fused_status): the `ol_wavefront_params` of the chief-ray reference
        sphere / plane for this field and wavelength (strategy.py:176-184, 228-243), from one
        traced chief ray."""
        t, rg = self.tracer, self.tracer.table.raygen
        hx, hy = self.field
        # The seven numbers of the traced chief ray come back in ONE device-to-host copy (its
        # status word is read with the fused launch's) and the reference geometry is worked
        # out on the host in double -- the same expressions as wavefront_device.h -- instead
        # of a one-ray kernel launch and four more read-backs
        fused_status = self.fused and hasattr(t, "defer_checks")
        if fused_status:
            t.defer_checks = True
        try:
            chief = t.trace_generic(hx, hy, 0.0, 0.0, self.wavelength)
        finally:
            if fused_status:
                t.defer_checks = False
        c = torch.stack([chief.x, chief.y, chief.z, chief.L, chief.M, chief.N, chief.opd]) \
            .reshape(7, -1)[:, 0].double().cpu().tolist()
        xc, yc, zc, Lc, Mc, Nc, opd_c = c
        ux, uy = self._tilt_cosines()
        params = dict(xc=xc, yc=yc, zc=zc, n_image=rg["n_image"], opd_ref=0.0, ux=ux,
                      uy=uy, half_epd=rg["EPD"] / 2.0, wavelength_um=self.wavelength)
        if self.afocal:  # strategy.py:260-284: plane through the chief-ray hit, normal to it
            R = math.inf
            params.update(R=0.0, nx=Lc, ny=Mc, nz=Nc)
            t_back = 0.0  # the chief ray starts ON its own plane
        else:
            R = math.sqrt(xc * xc + yc * yc + (zc - rg["pupil_z"]) ** 2)
            params.update(R=R)
            # back-propagation distance of the chief ray from the sphere's centre (its own
            # image point) to the sphere: the quadratic of reference_geometry.py:41-79
            # with r = centre -> c = -R^2, b = 0
            a_ = Lc * Lc + Mc * Mc + Nc * Nc
            sq = math.sqrt(max(4.0 * a_ * R * R, 0.0))
            t1, t2 = -sq / (2.0 * a_), sq / (2.0 * a_)
            t_back = t2 if t1 < 0.0 else t1
        # chief-ray OPD to the reference (pupil point (0, 0): no tilt term)
        params["opd_ref"] = opd_c - rg["n_image"] * t_back
        return params, R, fused_status

    def _compute(self) -> WavefrontData:
        if self.strategy != "chief_ray":
            return self._compute_fitted()
        t = self.tracer
        hx, hy = self.field
        # 1. chief ray alone -> reference sphere
        params, R, fused_status = self.chief_reference()
        # 2. the full pupil (strategy.py:190-205)
        if self.fused:  # one launch: pupil points -> OPD map + its reductions, no ray planes
            px, py = t._dev(self.distribution.x), t._dev(self.distribution.y)
            wl, _ = t._wavelength_index(self.wavelength)
            # (check_status=False keeps the chief-ray launches' status bits: one read-back
            # for the three launches)
            opd, intensity, pupil, mom = t.engine.trace_opd(
                params, px, py, wl, field=(hx, hy), vig=t._vig_scalar(hx, hy), want_pupil=True,
                check_status=not fused_status)
            if fused_status:
                t.check_status()
            return WavefrontData(pupil[0], pupil[1], pupil[2], opd, intensity, R, moments=mom)
        # the intensity the reference reads is the RECORDED image-plane row
        # (wavefront/strategy.py:198: surfaces.intensity[-1], i.e. before a polarised
        # update_intensity): record-all is forced for this trace whatever the caller set
        keep_record = t.record_all
        t.record_all = True
        try:
            rays = t.trace(hx, hy, self.wavelength, None, self.distribution)
            intensity = t.surfaces.intensity[-1].clone()
        finally:
            t.record_all = keep_record
        px = t._dev(self.distribution.x)
        py = t._dev(self.distribution.y)
        r7 = [v.contiguous() for v in (rays.x, rays.y, rays.z, rays.L, rays.M, rays.N, rays.opd)]
        opd, pupil = t.engine.wavefront_opd(params, r7, px, py, want_pupil=True)
        return WavefrontData(pupil[0], pupil[1], pupil[2], opd, intensity, R)


    def _compute_fitted(self) -> WavefrontData:
        """CentroidStrategy / BestFitStrategy (wavefront/strategy.py:287-620): the reference
        sphere / plane comes from the traced bundle itself -- centred on the intensity-weighted
        (3-sigma trimmed) centroid of the image points with the weighted mean wavefront
        distance as radius, or the least-squares sphere / plane through the wavefront points
        -- and the piston is the mean OPD of the rays with intensity > 0.  Three steps on the
        device: the trace, `ol_wavefront_fit` (a chain of reductions that leaves the reference
        in device memory) and `ol_wavefront_opd_fitted`; ONE read-back (radius + fit status).
        This stand-alone class follows the reference's NumPy backend where its two backends
        differ (np.std, plain mean)."""
        t, rg = self.tracer, self.tracer.table.raygen
        hx, hy = self.field
        rays = t.trace(hx, hy, self.wavelength, None, self.distribution)
        px, py = t._dev(self.distribution.x), t._dev(self.distribution.y)
        ux, uy = self._tilt_cosines()
        params = dict(n_image=rg["n_image"], wavelength_um=self.wavelength, ux=ux, uy=uy,
                      half_epd=rg["EPD"] / 2.0)
        r8 = [v.contiguous() for v in (rays.x, rays.y, rays.z, rays.L, rays.M, rays.N, rays.opd,
                                       rays.i)]
        px, py = px.contiguous(), py.contiguous()
        ref = t.engine.wavefront_fit(self.strategy, params, r8, px, py,
                                     trim_std=self.robust_trim_std, flavour="numpy",
                                     planar=self.afocal)
        opd, pupil = t.engine.wavefront_opd_fitted(ref, r8[:7], px, py, want_pupil=True)
        R, bits = t.engine.fit_result(ref)
        if bits & _capi.FIT_SINGULAR and self.strategy == "best_fit" and not self.afocal \
                and not bits & (_capi.FIT_NO_VALID | _capi.FIT_TOO_FEW):
            return self._best_fit_rank_deficient(r8, px, py, params)
        t.engine.raise_for_fit_status(bits)
        return WavefrontData(pupil[0], pupil[1], pupil[2], opd, r8[7].clone(),
                             math.inf if self.afocal else R)

    def _best_fit_rank_deficient(self, r8, px, py, params) -> WavefrontData:
        """The least-squares sphere through wavefront points that do not span space -- a
        collimated beam: the points of an afocal system lie in one plane -- the way the
        reference gets it (wavefront/strategy.py:556-582 on its NumPy backend):
        `np.linalg.lstsq` of the RAW system `[x y z 1] c = |p|^2`, i.e. the rank-3 minimum-norm
        solution of the SVD.  That sphere is an artefact of where the origin lies (4.7 mm of
        radius for a flat wavefront, hundreds of waves of "OPD"), but it is what the reference
        returns, so it is what this returns: the device fit reports the cloud as singular
        (`ol_wavefront_fit`: its centred normal equations have no fourth pivot), the points
        come back once, and the OPD map is taken on the device against the host's sphere
        (`ol_wavefront_opd`), piston = the mean over the rays with intensity > 0
        (strategy.py:331).  Rare by construction; `afocal=True` is the fit such a beam wants."""
        import numpy as np
        t = self.tracer
        x, y, z, L, M, N, opd, inten = (v.double().cpu().numpy() for v in r8)
        pxn, pyn = px.double().cpu().numpy(), py.double().cpu().numpy()
        ni, half = float(params["n_image"]), float(params["half_epd"])
        with np.errstate(all="ignore"):
            opd_t = opd + (params["ux"] * (pxn * half) + params["uy"] * (pyn * half))
            valid = (np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(L)
                     & np.isfinite(M) & np.isfinite(N) & np.isfinite(opd_t) & (inten != 0))
            pts = np.stack((x, y, z), axis=1)[valid] \
                - (opd_t[valid] / ni)[:, None] * np.stack((L, M, N), axis=1)[valid]
            A = np.concatenate([pts, np.ones((len(pts), 1))], axis=1)
            c = np.linalg.lstsq(A, (pts ** 2).sum(axis=1), rcond=None)[0]
            centre = c[:3] / 2
            R = float(np.sqrt(c[3] + (centre ** 2).sum()))
        sphere = dict(params, xc=float(centre[0]), yc=float(centre[1]), zc=float(centre[2]), R=R,
                      opd_ref=0.0)
        opd_w, pupil = t.engine.wavefront_opd(sphere, r8[:7], px, py, want_pupil=True)
        alive = r8[7] > 0
        if not bool(alive.any()):
            raise ValueError("No valid rays with non-zero intensity for OPD calculation.")
        opd_w = opd_w - opd_w[alive].mean()   # (piston - opd) / lambda, piston = mean(opd[i > 0])
        return WavefrontData(pupil[0], pupil[1], pupil[2], opd_w, r8[7].clone(), R)


class OPD(Wavefront):
    """wavefront/opd.py:72-93: OPD wavefront; `num_rays` = number of hexapolar rings for
    the default distribution (15), as in the reference (`num_rings` is kept as an alias)."""

    def __init__(self, tracer, field, wavelength, num_rays: int = 15,
                 distribution="hexapolar", strategy: str = "chief_ray",
                 remove_tilt: bool = False, num_rings: int | None = None, **kwargs):
        super().__init__(tracer, field, wavelength,
                         num_rays=num_rays if num_rings is None else num_rings,
                         distribution=distribution, strategy=strategy, remove_tilt=remove_tilt,
                         **kwargs)

    def rms(self) -> float:
        """opd.py:145-159."""
        d = self.data
        if d.moments is not None and d._moments_of is d.opd:
            cnt, _s1, s2 = d.moments[9:12].tolist()  # epilogue of the fused kernel, one read-back
            if cnt == 0:
                raise ValueError("No valid rays with non-zero intensity for RMS calculation.")
            return math.sqrt(s2 / cnt)
        mask = d.intensity > 0
        if not bool(mask.any()):
            raise ValueError("No valid rays with non-zero intensity for RMS calculation.")
        o = d.opd[mask]
        return float(torch.sqrt(torch.mean(o * o)))


class ZernikeOPD(OPD):
    """wavefront/zernike_opd.py:18-83: the Zernike decomposition of the OPD map over a hexapolar
    pupil, on the fused OPD of any of the three strategies and `ol_zernike_fit`.  Rays with
    intensity <= 0 are left out by the KERNEL (the reference's `mask`, without boolean indexing
    or a read-back).  `coeffs` (num_terms,) float64 device tensor, `poly(x, y)`, `indices`,
    `zernike_type`, `num_terms`; `x`, `y`, `z`: the fitted samples (all of them: the mask is
    `data.intensity > 0`)."""

    def __init__(self, tracer, field, wavelength, num_rings: int = 15,
                 zernike_type: str = "fringe", num_terms: int = 37, strategy: str = "chief_ray",
                 remove_tilt: bool = False, **kwargs):
        from . import zernike as Z

        self.num_terms = Z.check_terms(zernike_type, num_terms, "ZernikeOPD")
        self.zernike_type = zernike_type
        self.indices = Z.indices(zernike_type, self.num_terms)
        super().__init__(tracer, field, wavelength, num_rays=num_rings,
                         distribution="hexapolar", strategy=strategy, remove_tilt=remove_tilt,
                         **kwargs)
        self.x, self.y = tracer._dev(self.distribution.x), tracer._dev(self.distribution.y)
        self.z = self.data.opd
        self.num_pts = int(self.z.numel())
        self.coeffs, self.status = self._fit()
        if self.status:
            raise ValueError(f"ZernikeOPD: {Z.status_text(self.status)}")

    def _fit(self):
        """(coeffs, status): one `ol_zernike_fit` call and ONE read-back, the status word."""
        from .engine import zernike_fit

        c, status = zernike_fit(self.x, self.y, self.z, self.zernike_type, self.num_terms,
                                intensity=self.data.intensity, device=self.z.device)
        return c, int(status)

    def poly(self, x, y):
        """The fitted wavefront at normalised pupil points (`ol_zernike_eval`), in waves."""
        from .engine import zernike_eval

        return zernike_eval(self.coeffs, self.zernike_type, x, y, device=self.coeffs.device)


def calculate_grid_size(num_rays: int) -> tuple[int, int]:
    """psf/fft.py:20-39."""
    eff = int(np.floor(32 * 2 ** ((np.log2(num_rays) - 5) / 2)))
    return eff, num_rays * 2


def padded_pupil(wavefront, n: int, gsz: int) -> torch.Tensor:
    """The pupil function of a uniform-grid `wavefront` of n x n samples (psf/fft.py:101-137,
    copied by psf/mmdft.py:121-155): A exp(-i 2 pi OPD) on the disc, 0 off it, centred in a
    zeroed gsz x gsz complex128 grid (gsz = n: the pupil itself)."""
    d = wavefront.data
    # the disc mask comes from the SAME arithmetic that placed the traced samples
    # (distribution._uniform: np.linspace + np.meshgrid, row-major ravel) -- a
    # torch.linspace grid differs by an ulp on boundary points such as (0.6, 0.8)
    # and would select a different number of cells for many odd n
    g = np.linspace(-1.0, 1.0, n)
    xg, yg = np.meshgrid(g, g)
    cells = np.flatnonzero((xg**2 + yg**2 <= 1).reshape(-1)).astype(np.int32)
    before = (gsz - n) // 2
    eng = wavefront.tracer.engine
    if wavefront.fused and hasattr(eng, "pupil_fill"):
        cell = torch.from_numpy(cells).to(d.opd.device)
        return eng.pupil_fill(d.opd, d.intensity, cell, n, gsz)
    # un-fused path (polarised systems, other strategies, A/B): plain tensor ops
    P = torch.zeros(n * n, dtype=torch.complex128, device=d.opd.device)
    P[torch.from_numpy(cells.astype(np.int64)).to(d.opd.device)] = \
        torch.sqrt(d.intensity) * torch.exp(-2j * math.pi * d.opd)
    after = before + (gsz - n) % 2
    return torch.nn.functional.pad(P.reshape(n, n), (before, after, before, after))


class FFTPSF:
    """Scalar FFT PSF (psf/fft.py:42-262) for one field and wavelength."""

    def __init__(self, tracer, field, wavelength, num_rays: int = 128, grid_size=None,
                 strategy: str = "chief_ray", remove_tilt: bool = False, **kwargs):
        if grid_size is None:
            if num_rays < 32:
                raise ValueError("num_rays must be at least 32 if grid_size is not specified.")
            num_rays, grid_size = calculate_grid_size(num_rays)
        elif grid_size < num_rays:
            raise ValueError(f"Grid size ({grid_size}) must be greater than or equal to the "
                             f"number of rays ({num_rays}).")
        self.num_rays, self.grid_size = num_rays, grid_size
        self.wavefront = Wavefront(tracer, field, wavelength, num_rays, "uniform",
                                   strategy=strategy, remove_tilt=remove_tilt, **kwargs)
        self.pupil = self._generate_pupil()
        self.psf = self._compute_psf()

    def _generate_pupil(self) -> torch.Tensor:
        """psf/fft.py:101-137: A exp(-i 2 pi OPD) on the num_rays^2 grid, 0 off-disc --
        written straight into the zero-padded FFT grid by `ol_pupil_fill` (self._padded);
        the n x n block is returned as a view."""
        n, before = self.num_rays, (self.grid_size - self.num_rays) // 2
        self._padded = padded_pupil(self.wavefront, n, self.grid_size)
        return self._padded[before:before + n, before:before + n]

    def _compute_psf(self) -> torch.Tensor:
        """psf/fft.py:139-200: (padded pupil) FFT (rocFFT), |.|^2, Strehl normalisation."""
        amp = torch.fft.fftshift(torch.fft.fft2(self._padded))
        norm = float((self.pupil.abs() > 0).sum()) ** 2
        return (amp * amp.conj()).real / norm * 100

    def strehl_ratio(self) -> float:
        """psf/base.py:418-438."""
        c = self.psf.shape[0] // 2
        return float(self.psf[c, self.psf.shape[1] // 2]) / 100


MAX_FNUM = 10000.0  # utils.py:68


def working_fno(t, field, wavelength) -> float:
    """utils.py:45-106 get_working_FNO: chief ray + four marginal rays."""
    wl, _ = t._wavelength_index(wavelength)
    n = float(t.table.optics[-1, wl]["n2"])
    px = np.array([0.0, 0.0, 0.0, 1.0, -1.0])
    py = np.array([0.0, 1.0, -1.0, 0.0, 0.0])
    r = t.trace_generic(field[0], field[1], px, py, wavelength)
    L, M, N, i = (torch.as_tensor(v).double().reshape(-1).cpu().numpy()
                  for v in (r.L, r.M, r.N, r.i))
    dot = np.clip(L[0] * L[1:] + M[0] * M[1:] + N[0] * N[1:], -1.0, 1.0)
    na2 = (n * np.sin(np.arccos(dot))) ** 2
    valid = i[1:] > 0
    avg = float(np.mean(na2[valid] if valid.any() else na2))
    fno = math.inf if avg <= 0 else 1 / (2 * math.sqrt(avg))
    fno = min(fno, MAX_FNUM)
    if math.isnan(fno):
        raise ValueError("Working F/# could not be calculated due to raytrace errors.")
    return fno


class MMDFTPSF:
    """Matrix-multiply DFT PSF (psf/mmdft.py:19-283) for one field and wavelength: the PSF on
    `image_size` x `image_size` pixels of `pixel_pitch` um, straight from the num_rays^2 pupil of
    the device wavefront (no zero padding), by `ol_mmdft_psf`; a diffraction-limited system
    peaks at 100."""

    def __init__(self, tracer, field, wavelength, num_rays: int = 128, image_size=None,
                 pixel_pitch=None, strategy: str = "chief_ray", remove_tilt: bool = False,
                 **kwargs):
        # mmdft.py:72-118, to the letter
        if image_size is None and pixel_pitch is None:
            if num_rays < 32:
                raise ValueError("num_rays must be at least 32 if image_size and pixel_pitch are "
                                 "not specified.")
            num_rays, grid_size = calculate_grid_size(num_rays)
        self.tracer, self.num_rays = tracer, num_rays
        self.wavefront = Wavefront(tracer, field, wavelength, num_rays, "uniform",
                                   strategy=strategy, remove_tilt=remove_tilt, **kwargs)
        self.field, self.wavelength = self.wavefront.field, self.wavefront.wavelength
        clear_size = num_rays - 1
        if pixel_pitch is None:
            if image_size is None:
                image_size = grid_size
            pixel_pitch = self.wavelength * self.working_fno() * clear_size / image_size
        if image_size is None:   # the largest image of that pitch: the pad size, truncated
            image_size = int(self.wavelength * self.working_fno() * clear_size / pixel_pitch)
        self.image_size, self.pixel_pitch = image_size, pixel_pitch
        self.pupil = padded_pupil(self.wavefront, num_rays, num_rays)
        self.psf = self._compute_psf()

    def working_fno(self) -> float:
        """utils.py:45-106 get_working_FNO: chief ray + four marginal rays."""
        return working_fno(self.tracer, self.field, self.wavelength)

    def pad_size(self) -> float:
        """mmdft.py:239-245: the side of the zero-padded grid an FFT of this pitch would need."""
        return self.wavelength * self.working_fno() * (self.num_rays - 1) / self.pixel_pitch

    def _product(self, pupil, pad_size, image_size):
        from .engine import mmdft_psf
        return mmdft_psf(pupil, pad_size, image_size, device=pupil.device)

    def _compute_psf(self) -> torch.Tensor:
        """mmdft.py:157-177 and the check of :247-254."""
        pad_size = self.pad_size()
        if self.image_size > pad_size:
            raise ValueError(f"Supplied image_size of {self.image_size} not less than or equal to "
                             f"calculated pad size of {int(pad_size)}. Consider increasing "
                             "num_rays.")
        return self._product(self.pupil, pad_size, self.image_size)

    def strehl_ratio(self) -> float:
        """mmdft.py:203-221: the maximum (the PSF need not be centred in the image)."""
        return float(self.psf.max()) / 100


class HuygensPSF:
    """Scalar Huygens-Fresnel PSF (psf/huygens_fresnel.py:31-348 `ScalarHuygensPSF`) for one
    field and wavelength: the pupil samples of the device wavefront (uniform grid, fp64)
    summed onto a grid of image points by `ol_huygens_psf`, normalised to 100 at the peak of
    the ideal (zero-OPD, unit-amplitude) pupil.  Planar, unrotated image surfaces only: the
    drop-in (analysis_seams) takes its image points from the reference and covers the rest."""

    MAX_FNUM = MAX_FNUM

    def __init__(self, tracer, field, wavelength, num_rays: int = 128, image_size: int = 128,
                 strategy: str = "chief_ray", remove_tilt: bool = False, oversample=None,
                 pixel_pitch=None, normalization=None):
        self.tracer = tracer
        self.field = (float(field[0]), float(field[1]))
        self.wavelength = float(wavelength)
        self.num_rays, self.image_size = int(num_rays), int(image_size)
        self.oversample = oversample
        self.pixel_pitch = None if pixel_pitch is None else float(pixel_pitch)
        self.normalization = None if normalization is None else float(normalization)
        self.cx = self.cy = None
        self._image_origin = self._planar_image_surface()
        self.wavefront = Wavefront(tracer, self.field, self.wavelength, self.num_rays, "uniform",
                                   strategy=strategy, remove_tilt=remove_tilt)
        self.psf = self._compute_psf()

    def _planar_image_surface(self):
        from . import system as S
        s = self.tracer.table.surfaces[-1]
        plane = int(s["geom_kind"]) == S.GEOM_PLANE or (
            int(s["geom_kind"]) == S.GEOM_STANDARD and not math.isfinite(float(s["radius"])))
        if not plane or int(s["flags"]) & S.SURF_ROTATED:
            raise ValueError("HuygensPSF: the stand-alone class needs a planar, unrotated image "
                             "surface (use the reference's HuygensPSF through the drop-in)")
        return [float(v) for v in s["origin"]]

    def _sum(self, image, pupil, amp, opd_mm, Rp, device):
        from .engine import huygens_sum
        return huygens_sum(*image, *pupil, amp, opd_mm, self.wavelength * 1e-3, Rp,
                           device=device)

    def _determine_image_center(self):
        """huygens_fresnel.py:119-144: 6 hexapolar rings, rays with i > 0, image-local x / y."""
        rays = self.tracer.trace(self.field[0], self.field[1], self.wavelength, 6, "hexapolar")
        ok = rays.i > 0
        if not bool(ok.any()):
            return np.array([0.0]), np.array([0.0])
        ox, oy, _ = self._image_origin
        return ((rays.x[ok].double() - ox).cpu().numpy(),
                (rays.y[ok].double() - oy).cpu().numpy())

    def working_fno(self) -> float:
        """utils.py:45-106 get_working_FNO: chief ray + four marginal rays."""
        return working_fno(self.tracer, self.field, self.wavelength)

    def _get_image_extent(self):
        """huygens_fresnel.py:146-210."""
        rx, ry = self._determine_image_center()
        self.cx, self.cy = float(np.mean(rx)), float(np.mean(ry))
        wl_mm = self.wavelength * 1e-3
        if self.pixel_pitch is not None:
            extent = 0.5 * self.image_size * self.pixel_pitch
        else:
            if self.oversample is not None:
                f_cutoff = 1.0 / (self.working_fno() * wl_mm)
                self.pixel_pitch = 1.0 / (2 * self.oversample * f_cutoff)
                extent = 0.5 * self.image_size * self.pixel_pitch
            else:
                geometric = float(np.max(np.hypot(rx - self.cx, ry - self.cy)))
                ideal = 5.0 * self.working_fno() * 1.22 * wl_mm
                extent = max(geometric, ideal)
            self.pixel_pitch = 2 * extent / self.image_size
        return -extent + self.cx, extent + self.cx, -extent + self.cy, extent + self.cy

    def _get_image_coordinates(self, device):
        """huygens_fresnel.py:212-237 on a planar image surface (sag 0), local -> global."""
        xmin, xmax, ymin, ymax = self._get_image_extent()
        kw = dict(dtype=torch.float64, device=device)
        gx, gy = torch.meshgrid(torch.linspace(xmin, xmax, self.image_size, **kw),
                                torch.linspace(ymin, ymax, self.image_size, **kw), indexing="xy")
        ox, oy, oz = self._image_origin
        return gx + ox, gy + oy, torch.full_like(gx, oz)

    def _get_normalization(self, data, device) -> float:
        """huygens_fresnel.py:239-286: the ideal pupil's PSF at the on-axis image point."""
        if self.field != (0.0, 0.0):
            data = Wavefront(self.tracer, (0.0, 0.0), self.wavelength, self.num_rays,
                             "uniform").data
        kw = dict(dtype=torch.float64, device=device)
        point = [torch.zeros((1, 1), **kw), torch.zeros((1, 1), **kw),
                 torch.full((1, 1), self._image_origin[2], **kw)]
        psf = self._sum(point, (data.pupil_x, data.pupil_y, data.pupil_z),
                        torch.ones_like(data.intensity), torch.zeros_like(data.opd),
                        float(data.radius), device)
        return float(psf[0, 0])

    def _compute_psf(self) -> torch.Tensor:
        """huygens_fresnel.py:288-324."""
        d = self.wavefront.data
        device = d.opd.device
        wl_mm = self.wavelength * 1e-3
        image = self._get_image_coordinates(device)
        psf = self._sum(image, (d.pupil_x, d.pupil_y, d.pupil_z), torch.sqrt(d.intensity),
                        d.opd * wl_mm, float(d.radius), device)
        if self.normalization is None:
            self.normalization = self._get_normalization(d, device)
        return psf / self.normalization * 100.0

    def strehl_ratio(self) -> float:
        """psf/base.py:418-438."""
        return float(self.psf[self.psf.shape[0] // 2, self.psf.shape[1] // 2]) / 100
