"""gsss_logprob and gsss_gradient in EVERY exact-mode vector layout against the extended-precision reference
(tests/reference_math.py): every lane layout and the first and last dimension of every cooperative one, for every target
family -- vMF (K = 1, 3, 17), dense and diagonal Bingham, Fisher-Bingham, Uniform, curve-vMF (2 and 10 knots) and the generic
mixture -- on unit rows and on rows of norm 0.998 (HMC's leapfrog evaluates off the sphere), as rows and as a single point;
then the targets whose rows are read from global memory.

Bounds (the project's bar, TOL of test_hip_parity.py): |got - want| / max(1, |want|) < 1e-10 for log_prob, the same with the
row's |want|_inf as the scale for gradients.  The curve's gradient jumps between segments of equal distance: on a row whose two
best candidates differ in x.y by less than 64 d 2^-53 the device's gradient must be that of ONE of the tied candidates
(layout_cases.gradient_error); log_prob is continuous there and gets no allowance.  Nothing is left out."""
import numpy as np
import pytest

import layout_cases as lc
from layout_cases import gradient_error, rel

pytestmark = pytest.mark.gpu

TOL = 1e-10
LAYOUTS = ["lane2", "lane3", "lane4", "lane5", "lane6", "lane8", "lane10", "coop4x4", "coop4x8", "coop16x4", "coop16x8", "coop64x4",
           "coop64x8", "coop64x16", "coop64x32"]  # GSSS_VEC_LIST ids 1 .. 15


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    yield geosss_amd
    lc.release()  # the cached targets' device copies go with the module
    torch.cuda.synchronize()


def exact_kernel(pdf):
    return pdf._device_target().lib.gsss_kernel_name(pdf._device_target().handle, 0, 0, 0).decode()


def test_sweep_reaches_every_layout(gs):
    """Every layout the library selects for some d is reached by the sweep, at its first and its last dimension: a layout added
    to GSSS_VEC_LIST fails here until the sweep covers it."""
    lib = gs._lib.load()
    by_layout = {}
    d = 2
    while lib.gsss_exact_layout(d) > 0:
        by_layout.setdefault(lib.gsss_exact_layout(d), []).append(d)
        d += 1
    assert d - 1 == 2048 and sorted(by_layout) == list(range(1, len(LAYOUTS) + 1))
    for vec, dims in by_layout.items():
        assert dims[0] in lc.DIMS and dims[-1] in lc.DIMS, (LAYOUTS[vec - 1], dims[0], dims[-1])
    assert {lib.gsss_exact_layout(d) for d in lc.DIMS} == set(by_layout)


def check(pdf, X, ref, d, label):
    worst = {}
    for tag, P in (("unit", X), ("off", lc.OFF_SPHERE * X)):
        want_lp, want_gr = ref[tag]
        e = [rel(pdf._log_prob_device(P), want_lp), gradient_error(pdf, P, pdf._gradient_device(P), want_gr, d)]
        i = min(1, len(P) - 1)  # a single point (d,)
        e[0] = max(e[0], rel(pdf._log_prob_device(P[i]), want_lp[i]))
        e[1] = max(e[1], gradient_error(pdf, P[i:i + 1], pdf._gradient_device(P[i])[None], want_gr[i:i + 1], d))
        worst[tag] = e
    print(f"{label}: log_prob {worst['unit'][0]:.1e} / {worst['off'][0]:.1e}, gradient {worst['unit'][1]:.1e} / {worst['off'][1]:.1e}"
          " (unit rows / norm 0.998)")
    assert max(worst["unit"][0], worst["off"][0]) < TOL, ("log_prob", worst)
    assert max(worst["unit"][1], worst["off"][1]) < TOL, ("gradient", worst)


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("d", lc.DIMS)
def test_logprob_and_gradient(gs, d, family):
    pdf, X = lc.sweep_case(family, d)
    layout = LAYOUTS[gs._lib.load().gsss_exact_layout(d) - 1]
    if family == "gmix" and 65 <= d <= 128:
        layout = "coop64x4"  # three Bingham-type components of d + 1 rows do not fit coop16x8 (LAYOUT_CASES has one that does)
    assert f"<{layout}," in exact_kernel(pdf), exact_kernel(pdf)
    check(pdf, X, lc.reference("sweep", family, d), d, f"{family} d={d} {layout}")


@pytest.mark.parametrize("name", lc.LAYOUT_CASES)
def test_rows_in_global_memory(gs, name):
    """vMF means, knots and the mixture's component rows read from global memory (grad_t<true>, scan<true>, the all-global
    branch of Mixture::stage), and the move to the smallest sixty-four-lane layout where the natural one cannot hold the rows."""
    pdf, X, layout = lc.global_case(name)
    assert f"<{layout}," in exact_kernel(pdf), exact_kernel(pdf)
    check(pdf, X, lc.reference("global", name), pdf.d, f"{name} {layout}")
