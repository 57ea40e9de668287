"""`ol_huygens_psf` at the shapes where its launch geometry changes, and against the exact
field of tests/golden/exact_huygens.npz (tools/make_golden_exact.py: mpmath at 50 digits).

Shapes (against the NumPy fp64 direct sum, the tolerance of tests/test_gpu_huygens.py): image
counts around one and two tiles of 512 pixels and around the 256 lanes of a tile's first half;
pupil counts around one and two chunks of kMinChunk = 32; and 70 000 samples for one pixel,
where 2048 chunks of ceil(70000 / 2048) = 35 would leave the last 48 empty and the count is
recomputed to 2000.

Geometry (against the exact field): the kernel carries the phase in cycles with the low parts
of R and of 1 / lambda.  The bound, (n_pupil + 32) 2^-52 sum_j |a_j q_mj / R_mj| per pixel,
is summation rounding plus 32 ulp per term; the fp64 NumPy sum, whose k R is off by k R 2^-53
~ 1e-10 rad per term, misses it in every case of the fixture (the generator asserts that, and
stores by how much), so a kernel that lost those low parts would miss it too.  (It did: with
P - Q a plain fp64 difference the device stood at 111 x the bound in the golden geometry, where
NumPy stands at 179 x; half an ulp of P - Q is as much phase as half an ulp of R.)"""

import numpy as np
import pytest
import torch

from optiland_amd.engine import huygens_sum
from tests import _exact as E
from tests import _huygens as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = E.load("huygens")


def _sum(args, **kw):
    ix, iy, iz, px, py, pz, amp, opd, wl, rp = args
    planes = (torch.as_tensor(np.asarray(v), device=DEV) for v in (ix, iy, iz, px, py, pz, amp, opd))
    return huygens_sum(*planes, float(wl), float(rp), **kw)


@pytest.mark.parametrize("n_image,n_pupil", [(m, 97) for m in (255, 256, 257, 511, 512, 513, 1025)]
                         + [(3, n) for n in (1, 31, 32, 33, 63, 64, 65)] + [(1, 70000)])
def test_image_and_pupil_counts_around_the_tile_and_the_chunk(n_image, n_pupil):
    args = H.random_case(n_pupil, n_image, complex_amp=True, seed=1000 * n_image + n_pupil)
    want = H.direct_field(*args)
    psf, field = _sum(args, want_field=True)
    psf, field = psf.cpu().numpy(), field.cpu().numpy()
    peak = float(np.max(np.abs(want) ** 2))
    err_f = float(np.max(np.abs(field - want))) / np.sqrt(peak)
    err_p = float(np.max(np.abs(psf - np.abs(want) ** 2))) / peak
    # the same pixels, each computed alone: another tile position, lane and chunking
    alone = 0.0
    for m in sorted({0, n_image // 2, n_image - 1}):
        one = _sum(tuple(np.asarray(a)[m:m + 1] for a in args[:3]) + args[3:]).cpu().numpy()
        alone = max(alone, abs(float(one[0]) - float(psf[m])) / peak)
    print(f"\n[huygens shape] {n_image} pixels x {n_pupil} samples: field {err_f:.3e}, psf "
          f"{err_p:.3e} of the peak (bound 1e-9); alone {alone:.3e} (bound 1e-12)")
    assert psf.shape == (n_image,) and err_f <= 1e-9 and err_p <= 1e-9
    assert alone <= 1e-12


@pytest.mark.parametrize("case", E.names(GOLD, "cases"))
def test_geometries_against_the_exact_field(case):
    args = tuple(GOLD[f"{case}/{a}"] for a in H.ARGS)
    want, scale = GOLD[f"{case}/field"], GOLD[f"{case}/scale"]
    _psf, field = _sum(args, want_field=True)
    err = np.abs(field.cpu().numpy() - want)
    bound = E.huygens_bound(args[3].size, scale)
    host = GOLD[f"{case}/numpy_err"] / bound
    print(f"\n[huygens exact] {case}: {args[3].size} samples, lambda {float(args[8]):.4g} mm, "
          f"Rp {float(args[9]):.4g}: max |device - exact| / bound = {float((err / bound).max()):.3e} "
          f"(NumPy direct sum {host.min():.1f} ... {host.max():.1f})")
    assert float(host.max()) > 1.0
    assert np.all(err <= bound), (case, err, bound)
