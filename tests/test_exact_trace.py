"""The fused trace kernels against an exact trace of every surface kind they serve.

tests/golden/exact_trace.npz (tools/make_golden_exact_trace.py) holds, per case and dtype, the
inputs rounded to the dtype, their trace at 50 digits (tests/_exact_trace.py: a plain sequential
trace in mpmath, from the definitions of the surfaces) and the error of the SAME plain trace run
at the dtype's own precision -- the yardstick.  On the rays the truth keeps (no miss, clip or
total reflection, |cos incidence| >= 0.2), per recorded row and group:

    max |kernel - truth| <= 2 max(E_plain, eps scale)                        (fp64 and fp32)
    max |kernel - truth| <= 2 max(E_oracle, eps scale)                       (fp64)

plus, on and behind the rows they apply to, the terms of two documented rules: the Newton stop
rule with last-gradient reuse (tol on position and path, kappa tol on the direction, kappa the
largest second derivative of the sag over the bundle) and the conic normal taken from the hit's
own z (`_exact_trace.conic_normal_terms`).  The factor 2 stands for the scatter between the maxima
of two rounding sequences over ~130 rays and for the device's 1-ulp rcp / rsq / sqrt against
mpmath's correctly rounded ones; it is not measured on the code under test.  The second line says
that the kernels' deliberate deviations from the reference's formulae never lose to them.

`-m gpu`: the kernels on the MI355X; otherwise the same source built for the host
(tests/hostmath).  The measured ratios are in profiles/exact_trace.txt.
"""

import numpy as np
import pytest

from tests import _exact_trace as X

WHERE = [pytest.param("cuda", marks=pytest.mark.gpu), "host"]
FIX = X.load()


def _engine(where, name, tag):
    eng = X.engine_for(where, X.case_table(name, tag))
    if eng is None:
        pytest.skip("hipcc (used as host C++ compiler) missing")
    return eng


def _report(label, err, lim):
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    k, g = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"\n[exact trace] {label}: worst error / bound {ratio.max():.2f} "
          f"(row {k}, {X.GROUPS[g]}: {err[k, g]:.3e} against {lim[k, g]:.3e})")
    return ratio


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", X.TAGS)
@pytest.mark.parametrize("name", X.CASES)
def test_record_against_the_exact_trace(name, tag, where):
    eng = _engine(where, name, tag)
    got = X.run_kernel(eng, FIX[f"{name}/{tag}/in"])
    eng.close()
    truth, keep = X.truth_of(FIX, name, tag), FIX[f"{name}/{tag}/keep"]
    assert got.shape == truth.shape
    assert np.array_equal(np.isnan(got[:, :, keep]), np.isnan(truth[:, :, keep]))
    assert np.array_equal(got[:, 6, keep] == 0, truth[:, 6, keep] == 0)
    err, plain, ref = X.compare(FIX, name, tag, got)
    ratio = _report(f"{name} {tag} {where} vs plain", err, plain)
    assert np.all(err <= plain), np.argwhere(ratio > 1)
    if ref is not None:
        ratio = _report(f"{name} {tag} {where} vs oracle", err, ref)
        assert np.all(err <= ref), np.argwhere(ratio > 1)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", X.TAGS)
@pytest.mark.parametrize("name", X.CASES)
def test_written_back_state_against_the_exact_trace(name, tag, where):
    """record=False: the state the launch writes back into the ray planes is the truth's last
    row under that row's bound.  (Every other launch variant is tied to the recording one bit
    for bit by test_every_kernel_variant_is_bit_identical.)"""
    eng = _engine(where, name, tag)
    got = X.run_kernel(eng, FIX[f"{name}/{tag}/in"], record=False)
    eng.close()
    truth, keep = X.truth_of(FIX, name, tag), FIX[f"{name}/{tag}/keep"]
    assert not np.isnan(got[:, keep]).any() and np.all(got[6, keep] != 0)
    full = np.where(np.arange(truth.shape[0])[:, None, None] == truth.shape[0] - 1, got[None],
                    truth)
    err, plain, ref = X.compare(FIX, name, tag, full)
    _report(f"{name} {tag} {where} write-back", err[-1:], plain[-1:])
    assert np.all(err[-1] <= plain[-1])
    if ref is not None:
        assert np.all(err[-1] <= ref[-1])
