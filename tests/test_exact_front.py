"""Ray generation and the fused spot, chief-reference and OPD kernels against exact truth.

tests/golden/exact_front.npz (tools/make_golden_exact_front.py) holds, per case, the inputs
(rounded to fp32 once: the same numbers are every dtype's inputs), what the reference's formulae
give for them at 50 digits (tests/_exact_front.py, with `_exact_trace.trace_ray` between ray
generation and the image) and the error of the SAME plain formulae at 53 / 24 bits, E_plain.
Nothing below -- no factor, floor or term -- was taken from the kernels; every comparison prints
its error / bound, and profiles/exact_front.txt holds the measured ratios.

1. Generated rays (`ol_generate_rays`, launch-uniform and per-ray field / vignetting planes), per
   group: max |kernel - truth| <= 2 max(E_plain, eps scale); scale = the largest |coordinate|
   (z_first - offset included) for the position, 1 for direction and intensity.  The apodised
   intensity's yardstick is max(E_plain, E_numpy), E_numpy the error of the reference's own NumPy
   line at the dtype: mpmath's exp / cos / pow are correctly rounded, a library's are not.  The
   status word equals the truth's.
2. The generating trace (`ol_trace_generate`): every recorded row against the truth TRACED FROM
   THE TRUE GENERATED RAYS, under `_exact_trace.bound` with the end-to-end yardstick (generate,
   then trace, at the working precision), the Newton / conic-normal terms of the exact trace and
   the lever term of those two rules on the position (below).
3. Spot hits (`ol_trace_spot`): the image-row bound of 2.  Spot moments about (0, 0) and about
   the truth's centroid rounded to the dtype: the count is exact -- the fixture keeps every truth
   hit farther from an aperture edge than the fp32 position bound of its row -- and with
   b = b_pos + eps |dx| (the image-row bound, plus the rounding of x - cx at the dtype: the
   yardstick's own) every sum is within the triangle-inequality image of the per-ray bounds:
       |sum dx - truth|   <= sum b                  (each term is off by at most b)
       |sum dx^2 - truth| <= sum (2 |dx| b + b^2)   ((dx + e)^2 - dx^2 = 2 dx e + e^2)
       |sum i - truth|    <= n b_i
       |max r^2 - truth|  <= 2 r_max b2 + b2^2, b2 = sqrt(2) b   (two coordinates off by b each
                             move the hit by at most sqrt(2) b; the largest of n numbers moves by
                             no more than the largest move)
   each plus n 2^-52 times the sum of the terms' magnitudes for the fp64 accumulation of n terms
   in any order.  Asking for the hit planes or not gives the same count and max r^2 exactly.
4. Chief reference (`ol_wavefront_reference`), sphere and forced plane: centre and returned chief
   ray under 2 max(E_plain, eps scale) of their group (+ the exact trace's rule terms at the image
   row: e_pos, e_dir, e_path); R likewise with sqrt(3) e_pos (R moves by at most the centre's
   move); opd_ref = path - n R with e_path + n sqrt(3) e_pos; the plane's normal under the
   direction bound.
5. OPD in waves per ray: |kernel - truth| <= 2 max(E_plain, eps S), S = max(|path|, n_image R,
   |opd_ref|) / wavelength -- one rounding of the longest length in the chain -- plus the rule
   terms carried into t: (e_path + n_image (H e_pos + G e_dir)) / wavelength.  With u = r - c and
   e the backward direction, t = -(u.e) + sqrt((u.e)^2 - |u|^2 + R^2), so |dt/dr| <= 1 +
   |u| / sqrt(R^2 - |u|^2) =: H and |dt/de| <= |u| H =: G; for the plane t = -(u.n) / (e.n):
   H = 1 / |e.n|, G = |u| / (e.n)^2.  Reference-surface points r - t d: 2 max(E_plain, eps
   max(|t|, |coordinate|)) + e_pos + (H e_pos + G e_dir) + |t| e_dir.  Three paths:
   (a) `ol_trace_opd` with the truth's reference rounded to fp64 as input; (b)
   `ol_wavefront_reference` then `ol_trace_opd_dev`: the truth is the one from the TRUE chief
   ray, the yardstick includes the plain chief reference, and the chief ray's share of the rule
   terms is added once more; (c) the stand-alone `ol_wavefront_opd` on the truth's image rays
   rounded to fp64: the bound of that step alone, no rule terms.
6. OPD moments: counts exact; every sum of products w od X ... within sum (prod (|v| + b_v) -
   prod |v|) over the per-ray bounds of 3 and 5 -- the triangle inequality on a product -- plus
   n 2^-52 relative.

The two-rays-per-lane OPD form starts at 2^20 rays and is tied bit for bit to the one-ray form
by test_fused_opd_two_rays_per_lane_is_bit_identical, so these sizes (132 / 264 rays: two tiles,
the second ragged) serve it too.  The host leg runs the shared device functions through
tests/hostmath, whose harness restates the launch loops: indexing, tails, wave reductions and
atomics are tested by the `cuda` leg only.  Where these bounds hold, the tolerances of
tests/test_wavefront.py (1e-7, 2e-7 scale, 1e-9 scale against fp64 oracle numbers) and the
1e-5 / 1e-10 / rtol 1e-9 of the spot-moment tests are redundant; those tests stay as they are.

THE LEVER TERM.  With the bound of 2 as the exact trace states it, one table misses on the host
and on the MI355X alike: finite_object_height_telecentric_generic, whose object is 150 mm in
front of the first surface and whose image plane 62 mm behind the last -- image-row position
1.07 of the bound (fp32: trace and spot hits), reference-plane points 1.60 (fp64, axis field).
The same source built with the reference's conic normal (from x, y instead of the hit's own z)
meets every bound here without it (worst 0.92), so the cause is that documented rule,
whose term the exact trace carries in the DIRECTION only: after 150 mm all of the hit's error is
in z, the normal follows it, and the steps behind carry the turned direction into the hits.
`_exact_front.trace_bound` therefore adds, to the position bound alone, what the allowed
direction deviation of the two rules does to the next hit, t / cos per unit turn, carried on
from row to row (derivation there); the reference-surface points and the chief ray's hit take
the image row's term (+ last thickness x e_dir).  The OPD in waves takes none: a turn at a
surface changes the path to second order only (Fermat), and the bound of 5 holds as it is.  The
term is derived from the truth (steps, cosines, the rule's own direction term), not measured on
the kernels; no factor changed.
"""

import numpy as np
import pytest

from tests import _exact_front as F

WHERE = [pytest.param("cuda", marks=pytest.mark.gpu), "host"]


def _report(label, checks):
    if checks is None:
        pytest.skip("hipcc (used as host C++ compiler) missing")
    ratios = np.array([F.ratio_of(e, b) for _, e, b in checks])
    k = int(np.argmax(ratios))
    print(f"\n[exact front] {label}: worst error / bound {ratios[k]:.2f} "
          f"({checks[k][0]}: {checks[k][1]:.3e} against {checks[k][2]:.3e})")
    for lab, e, b in checks:
        print(f"    {lab:32s} {e:.3e} / {b:.3e} = {F.ratio_of(e, b):.2f}")
    return [(lab, e, b) for lab, e, b in checks if not e <= b]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", F.TAGS)
@pytest.mark.parametrize("name", list(F.GEN_CASES))
def test_generated_rays_against_the_exact_generator(name, tag, where):
    assert not _report(f"generate {name} {tag} {where}", F.check_generate(where, name, tag))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", F.TAGS)
def test_status_word_of_out_of_range_points(tag, where):
    assert not _report(f"status {tag} {where}", F.check_status(where, tag))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", F.TAGS)
@pytest.mark.parametrize("name", list(F.TRACE_CASES))
def test_generating_trace_against_the_truth_from_true_rays(name, tag, where):
    assert not _report(f"trace {name} {tag} {where}", F.check_trace(where, name, tag))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", F.TAGS)
@pytest.mark.parametrize("name", list(F.TRACE_CASES))
def test_spot_hits_and_moments_against_exact_sums(name, tag, where):
    assert not _report(f"spot {name} {tag} {where}", F.check_spot(where, name, tag))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", list(F.TRACE_CASES))
def test_chief_reference_against_the_exact_reference(name, where):
    assert not _report(f"chief {name} {where}", F.check_chief(where, name))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("kind", F.REFS)
@pytest.mark.parametrize("f", (0, 1))
@pytest.mark.parametrize("name", list(F.TRACE_CASES))
def test_opd_points_and_moments_against_the_exact_wavefront(name, f, kind, where):
    assert not _report(f"opd {name} field {f} {kind} {where}", F.check_opd(where, name, f, kind))
