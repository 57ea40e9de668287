"""`ol_mmdft_psf` against the exact transform of tests/golden/exact_mmdft.npz
(tools/make_golden_exact_mmdft.py: mpmath at 50 digits, rounded to fp64 once).

The bound is rounding analysis of the kernel's own operations (tests/_mmdft.py): two N-term
complex sums and a table entry good to 3 ulp, B = (2 N + 8) 2^-52 sum |g| for the field and
(2 |G| B + B^2) 100 / c^2 for the PSF.  The cases: one cell; M < N with a non-integer pad; the
sizes of the golden cases (odd N, a non-integer pad, more than one tile of 64); M < N at a full
tile."""

import numpy as np
import pytest
import torch

from optiland_amd.engine import mmdft_psf
from tests import _mmdft as MM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = MM.exact()


@pytest.mark.parametrize("case", MM.cases(GOLD))
def test_field_and_psf_against_the_exact_transform(case):
    pupil, pad = GOLD[f"{case}/pupil"], float(GOLD[f"{case}/pad_size"])
    m, n = int(GOLD[f"{case}/image_size"]), pupil.shape[0]
    sum_abs, c = float(GOLD[f"{case}/sum_abs"]), int(GOLD[f"{case}/count"])
    psf, field = mmdft_psf(torch.as_tensor(pupil, device=DEV), pad, m, want_field=True)
    err_f = np.abs(field.cpu().numpy() - GOLD[f"{case}/field"])
    err_p = np.abs(psf.cpu().numpy() - GOLD[f"{case}/psf"])
    b = MM.field_bound(n, sum_abs)
    bp = MM.psf_bound(n, sum_abs, GOLD[f"{case}/field"], c)
    host = float(GOLD[f"{case}/numpy_field_err"])
    print(f"\n[mmdft exact] {case}: N {n}, M {m}, pad {pad!r}: max |G_dev - G_exact| / B = "
          f"{err_f.max() / b:.3e} (NumPy formula {host / b:.3e}), worst |psf_dev - psf_exact| / "
          f"bound = {float((err_p / bp).max()):.3e}")
    assert err_f.shape == (m, m)
    assert np.all(err_f <= b), (case, float(err_f.max()), b)
    assert np.all(err_p <= bp), case
