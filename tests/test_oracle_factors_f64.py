"""Pins K11 / K12 / the IRLS weights of the CPU oracle for EVERY factor and EVERY robust loss against the float64 model of
tests/f64_factors.py (finite differences of the cost, of the residual and of rho; written from the mathematics, not from the
oracle's or the kernels' code). tests/test_oracle_gicp_f64.py does this for GICP and point-to-distribution without a robust loss;
this file adds POINT_TO_POINT, POINT_TO_PLANE, GENZ (class, weight g), HUBER, TUKEY, CAUCHY, GEMAN_MCCLURE (rho, w = rho' / r).

Tolerance: the 2e-4 relative to max|H64|, max|b64| and the error that test_oracle_gicp_f64.py holds the oracle to. `pytest -s`
prints the measured distances per pair (the table in DESIGN.md section 2)."""
import numpy as np
import pytest

import f64_factors as f64

TOL = 2e-4
N = 300


@pytest.fixture(scope="module")
def case():
    c = f64.make_case(N, N)
    assert 0.8 * N < c.inliers.sum() < 0.9 * N  # about 1 in 7 rejected
    return c


@pytest.fixture(scope="module")
def scales(case):
    return {f: f64.robust_scale(case, f) for f in f64.FACTORS}


def test_fast_path_equals_finite_difference_path(case, scales):
    # before anything else uses system_fast: the analytic J = [R skew(p) | -R] against central differences, every pair
    for factor in f64.FACTORS:
        for loss in f64.LOSSES:
            a = f64.system_fd(case, factor, loss, scales[factor])
            b = f64.system_fast(case, factor, loss, scales[factor])
            d = f64.distances(b["H"], b["b"], b["error"], a)
            # 1e-6: the step of the differences. (The scale is the median residual norm, so one point sits ON the kink of
            # HUBER's and TUKEY's second derivative, where a central difference of the cost is off by O(step): 1.2e-7 measured.)
            assert max(d.values()) <= 1e-6, (factor, loss, d)
            assert a["inlier"] == b["inlier"] and np.array_equal(a["w"], b["w"])


def test_finite_difference_weight_is_the_published_irls_weight(case):
    # the model's w against the textbook closed forms (Zhang, "Parameter estimation techniques", table 1), which neither the
    # model nor its users compute anywhere else: guards the model's rho
    r, s = np.linspace(0.05, 3.0, 60), 1.3
    x = (r / s) ** 2
    closed = {"NONE": np.ones_like(r), "HUBER": np.minimum(1.0, s / r), "TUKEY": np.where(r < s, (1 - x) ** 2, 0.0),
              "CAUCHY": 1 / (1 + x), "GEMAN_MCCLURE": 1 / (1 + x) ** 2}
    for loss in f64.LOSSES:
        assert np.abs(f64.irls_weight_fd(loss, r, s) - closed[loss]).max() <= 1e-5, loss


@pytest.mark.parametrize("loss", f64.LOSSES)
@pytest.mark.parametrize("factor", f64.FACTORS)
def test_oracle_system_matches_float64_model(orc, case, scales, factor, loss):
    s = scales[factor]
    ref = f64.system_fd(case, factor, loss, s)
    args = (case.src, case.scov, case.tgt, case.tcov, case.nrm, case.nn, case.d2, case.T, case.max_corr, factor, loss, s)
    res = orc.gicp_linearize(*args, case.alpha)
    assert res["inlier"] == ref["inlier"] == int(case.inliers.sum())
    hs, bs = np.abs(ref["H"]).max(), np.abs(ref["b"]).max()
    dH, db = np.abs(res["H"] - ref["H"]).max() / hs, np.abs(res["b"] - ref["b"]).max() / bs
    de11 = abs(res["error"] - ref["error"]) / ref["error"]
    e12, c12 = orc.gicp_error(*args, case.alpha)  # K12 at the same pose: the same error, the same count
    de12 = abs(e12 - ref["error"]) / ref["error"]
    print(f"\n[oracle-f64] {factor:22s} {loss:14s} H {dH:.1e}  b {db:.1e}  K11 error {de11:.1e}  K12 error {de12:.1e}", end="")
    assert dH <= TOL and db <= TOL and de11 <= TOL
    assert c12 == ref["inlier"] and de12 <= TOL


@pytest.mark.parametrize("loss", f64.LOSSES)
@pytest.mark.parametrize("factor", [f for f in f64.FACTORS if f != "GENZ"])
def test_oracle_irls_weights_match_finite_difference_of_rho(orc, case, scales, factor, loss):
    s = scales[factor]
    ref = f64.system_fd(case, factor, loss, s)
    w = orc.icp_robust_weights(case.src, case.scov, case.tgt, case.tcov, case.nrm, case.nn, case.d2, case.T, case.max_corr,
                               factor, loss, s)
    want = np.zeros(N)  # a rejected correspondence weighs nothing (registration.hpp:441-458)
    want[ref["index"]] = ref["w"]
    if loss == "TUKEY":  # both branches populated (robust_scale asserts a quarter of the inliers on each side of the scale)
        assert (ref["w"] == 0.0).sum() >= N // 5 and (ref["w"] > 0.0).sum() >= N // 5
    dw = np.abs(w - want).max()
    print(f"\n[oracle-f64] {factor:22s} {loss:14s} w {dw:.1e}", end="")
    assert dw <= TOL  # weights are in [0, 1]: absolute
