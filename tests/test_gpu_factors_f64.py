"""Every (factor, robust loss) pair the library compiles, on every kernel path, against the float64 model of tests/f64_factors.py
(finite differences of the cost, the residual and rho, written from the mathematics) AND against the CPU oracle:

  (a) the generic kernels (sp_gicp_linearize, sp_gicp_error, sp_icp_robust_weights): 5 factors x 5 losses;
  (b) the same kernels at the sizes where a reduction goes wrong: one point, partial waves, partial 256-lane workgroups, several
      workgroups, every correspondence rejected, a single inlier at the last index;
  (c) the prepared / fused kernels (sp_gicp_iteration_fused, sp_gicp_error_prepared, the linearisation step of
      sp_gicp_align_optimize): GICP and POINT_TO_DISTRIBUTION x 5 losses, correspondences found by the kernel itself.

Two bounds, both PER 3x3 BLOCK of H (rotation, translation, coupling) and per half of b, each relative to that block's own float64
maximum — a wrong coupling block that is small beside the largest entry of H does not pass:
  * against float64: 2e-4, what tests/test_oracle_factors_f64.py holds the oracle itself to;
  * against the oracle: 2e-5, the bound of every other kernel-against-oracle test of this suite.
The per-point IRLS weights lie in [0, 1] and are held absolutely: 2e-4 against the finite difference of rho and, against the oracle,
the 2e-4 test_gpu_parity.py::test_linearize_error_weights_match_oracle already uses (the GICP / point-to-distribution norms go
through acosf / cosf).

`pytest -s` prints the measured maxima per (path, factor, loss): the table in DESIGN.md section 2."""
import ctypes as C

import numpy as np
import pytest

import f64_factors as f64

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL_F64 = 2e-4
TOL_ORACLE = 2e-5
TOL_WEIGHT = 2e-4


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def case300():
    return f64.make_case(300, 300)


@pytest.fixture(scope="module")
def scales300(case300):
    return {f: f64.robust_scale(case300, f) for f in f64.FACTORS}


def oracle_args(case, factor, loss, scale):
    return (case.src, case.scov, case.tgt, case.tcov, case.nrm, case.nn, case.d2, case.T, case.max_corr, factor, loss, scale)


def lin_result(got):
    return np.array(got.H, np.float32).reshape(6, 6), np.array(got.b, np.float32), float(got.error), int(got.inlier)


def hold(tag, H, b, error, inlier, ref64, oref):
    """The two bounds, per block; prints what was measured before it asserts."""
    d64 = f64.distances(H, b, error, ref64)
    dor = f64.distances(H, b, error, oref, ref64)
    print(f"\n[gpu-f64] {tag:64s} f64 {max(d64.values()):.1e}  oracle {max(dor.values()):.1e}", end="")
    assert inlier == ref64["inlier"] == oref["inlier"], tag
    assert np.array_equal(H, H.T), tag
    assert max(d64.values()) <= TOL_F64, (tag, d64)
    assert max(dor.values()) <= TOL_ORACLE, (tag, dor)


class GenericPath:
    """Registration._linearize / compute_error_frozen / compute_icp_robust_weights over given correspondences, as
    test_gpu_parity.py::test_linearize_error_weights_match_oracle drives them."""

    def __init__(self, sp, case, factor, loss):
        self.sp, self.case = sp, case
        self.reg = sp.Registration(sp.RegistrationParams(reg_type=factor, robust_type=loss, max_correspondence_distance=case.max_corr))
        self.reg.genz_alpha = case.alpha
        self.S = sp.PointCloudShared(dev(case.src), covs=dev(case.scov))
        self.Tg = sp.PointCloudShared(dev(case.tgt), covs=dev(case.tcov), normals=dev(case.nrm))
        self.reg.neighbors.indices, self.reg.neighbors.distances = dev(case.nn.reshape(-1, 1)), dev(case.d2.reshape(-1, 1))

    def linearize(self, scale):
        _, lin = self.reg._buffers(self.S.points.device)
        self.reg._linearize("linearize", self.S, self.Tg, self.case.T, scale, lin)
        return self.reg._read_lin(lin)

    def error(self, scale):
        return self.reg.compute_error_frozen(self.S, self.Tg, self.case.T, scale)

    def weights(self, scale):
        sp, case = self.sp, self.case

        class Frozen(sp.KNNBase):
            def knn_search_async(self, queries, k, result, transT=None):
                result.indices, result.distances = dev(case.nn.reshape(-1, 1)), dev(case.d2.reshape(-1, 1))

        return self.reg.compute_icp_robust_weights(self.S, self.Tg, Frozen(), case.T, scale).cpu().numpy()


def check_generic(sp, orc, case, factor, loss, scale, ref64, tag):
    oref = orc.gicp_linearize(*oracle_args(case, factor, loss, scale), case.alpha)
    path = GenericPath(sp, case, factor, loss)
    got = path.linearize(scale)
    H, b, error, inlier = lin_result(got)
    hold(tag + " K11", H, b, error, inlier, ref64, oref)
    again = path.linearize(scale)  # deterministic reduction: a second launch gives the same bits
    assert bytes(again)[:176] == bytes(got)[:176], tag
    e12, c12 = path.error(scale)
    oe12, oc12 = orc.gicp_error(*oracle_args(case, factor, loss, scale), case.alpha)
    assert c12 == oc12 == ref64["inlier"], tag
    d64, dor = f64.relative(abs(e12 - ref64["error"]), ref64["error"]), f64.relative(abs(e12 - oe12), ref64["error"])
    print(f"  K12 f64 {d64:.1e}  oracle {dor:.1e}", end="")
    assert d64 <= TOL_F64 and dor <= TOL_ORACLE, (tag, d64, dor)
    return path


# ------------------------------------------------------------------ (a) generic kernels, every pair
@pytest.mark.parametrize("loss", f64.LOSSES)
@pytest.mark.parametrize("factor", f64.FACTORS)
def test_generic_kernels_match_float64_and_oracle(sp, orc, case300, scales300, factor, loss):
    case, s = case300, scales300[factor]
    ref64 = f64.system_fd(case, factor, loss, s)
    path = check_generic(sp, orc, case, factor, loss, s, ref64, f"generic n=300 {factor} {loss}")
    if factor != "GENZ":  # registration.hpp:279-294 computes no GENZ weight
        w = path.weights(s)
        want = np.zeros(len(case.src))  # a rejected correspondence weighs nothing
        want[ref64["index"]] = ref64["w"]
        ow = orc.icp_robust_weights(*oracle_args(case, factor, loss, s))
        d64, dor = float(np.abs(w - want).max()), float(np.abs(w - ow).max())
        print(f"  w f64 {d64:.1e}  oracle {dor:.1e}", end="")
        assert d64 <= TOL_WEIGHT and dor <= TOL_WEIGHT, (factor, loss, d64, dor)


# ------------------------------------------------------------------ (b) size sweep
SWEEP_PAIRS = [("GICP", "TUKEY"), ("GENZ", "HUBER")]
SWEEP_SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097]  # wave (64) and workgroup (256) edges, one multi-block size


def sweep_scale(case, factor, scales300):
    """The scale of the n = 300 case (same generator, same distribution): both branches of the loss stay populated, which is
    asserted from 63 points on. With a handful of inliers, twice their largest residual norm instead: a lone point beyond TUKEY's
    scale would make every sum exactly zero and the case would check nothing."""
    rn = f64.residual_norms(case, factor)
    if len(rn) < 8:
        return float(np.float32(2.0 * rn.max()))
    s = scales300[factor]
    assert (rn < s).mean() >= 0.25 and (rn > s).mean() >= 0.25
    return s


@pytest.mark.parametrize("n", SWEEP_SIZES)
@pytest.mark.parametrize("factor,loss", SWEEP_PAIRS)
def test_generic_kernels_size_sweep(sp, orc, scales300, factor, loss, n):
    case = f64.make_case(n, 300, seed=1000 + n)
    s = sweep_scale(case, factor, scales300)
    ref64 = f64.system_fast(case, factor, loss, s)
    assert ref64["inlier"] == n - len(range(3, n, 7)) and np.abs(ref64["H"]).max() > 0.0
    check_generic(sp, orc, case, factor, loss, s, ref64, f"sweep n={n} {factor} {loss}")


@pytest.mark.parametrize("factor,loss", SWEEP_PAIRS)
def test_generic_kernels_every_correspondence_rejected(sp, scales300, factor, loss):
    case = f64.make_case(1025, 300, seed=77)
    case = case.with_correspondences(case.nn, np.full(1025, f64.REJECTED_D2, np.float32))
    path = GenericPath(sp, case, factor, loss)
    H, b, error, inlier = lin_result(path.linearize(scales300[factor]))
    assert inlier == 0 and error == 0.0 and not H.any() and not b.any()
    assert path.error(scales300[factor]) == (0.0, 0)


@pytest.mark.parametrize("factor,loss", SWEEP_PAIRS)
def test_generic_kernels_single_inlier_at_the_last_index(sp, orc, scales300, factor, loss):
    n = 1025  # the inlier is the only point of the last workgroup
    case = f64.make_case(n, 300, seed=78, reject_every=0)
    d2 = np.full(n, f64.REJECTED_D2, np.float32)
    d2[-1] = case.d2[-1]
    case = case.with_correspondences(case.nn, d2)
    s = sweep_scale(case, factor, scales300)
    ref64 = f64.system_fast(case, factor, loss, s)
    assert ref64["inlier"] == 1 and ref64["index"][0] == n - 1 and np.abs(ref64["H"]).max() > 0.0
    check_generic(sp, orc, case, factor, loss, s, ref64, f"single inlier n={n} {factor} {loss}")


# ------------------------------------------------------------------ (c) prepared / fused kernels
N_TARGET = 3000
TRIALS = ([0.0] * 6, [0.002, 0.001, -0.003, 0.01, 0.02, -0.01], [-0.01, 0.004, 0.002, -0.03, 0.0, 0.02])


class PreparedPath:
    """PreparedTarget over the synthetic target and its covariances, a prepared source, the library's own search."""

    def __init__(self, sp, case, factor, loss, fast_nn=None):
        self.sp, self.case, self.factor = sp, case, factor
        self.L = sp._lib.lib()
        self.S = sp.PointCloudShared(dev(case.src), covs=dev(case.scov))
        self.prep = sp.PreparedTarget(sp.GridKNN.build(dev(case.tgt)), dev(case.tcov), reg_type=factor)
        self.reg = sp.Registration(sp.RegistrationParams(reg_type=factor, robust_type=loss, max_correspondence_distance=case.max_corr))
        self.psrc = sp.PreparedSource(len(case.src))
        if fast_nn is not None:
            self.psrc._set_option("fast_nn", fast_nn)  # csrc/sp_internal.h: per-handle, nothing to restore
        self.psrc.prepare(self.prep, self.S, case.T, sort_by_cell=True)
        self.Tl = np.ascontiguousarray(case.T.T).reshape(-1)

    def iteration_fused(self, scale):
        sp, reg = self.sp, self.reg
        ws, lin = reg._buffers(self.S.points.device)
        fp = reg._factor_params(scale)
        reg.neighbors.resize(len(self.case.src), 1, self.S.points.device)
        sp.check(self.L.sp_gicp_iteration_fused(self.prep._h, self.psrc._h, self.Tl.ctypes.data_as(C.c_void_p), 0, C.byref(fp), None,
                                                sp._ptr(reg.neighbors.indices), sp._ptr(reg.neighbors.distances), sp._ptr(lin), None,
                                                sp._ptr(ws), ws.numel(), sp._stream()))
        got = reg._read_lin(lin)
        return got, reg.neighbors.indices.cpu().numpy().reshape(-1), reg.neighbors.distances.cpu().numpy().reshape(-1)

    def error_prepared(self, scale, T_trial):
        sp, reg = self.sp, self.reg
        ws, lin = reg._buffers(self.S.points.device)
        fp = reg._factor_params(scale)
        Tt = np.ascontiguousarray(np.asarray(T_trial, np.float32).T).reshape(-1)
        sp.check(self.L.sp_gicp_error_prepared(self.prep._h, self.psrc._h, self.Tl.ctypes.data_as(C.c_void_p),
                                               Tt.ctypes.data_as(C.c_void_p), 0, C.byref(fp), sp._ptr(lin), sp._ptr(ws), ws.numel(),
                                               sp._stream()))
        got = reg._read_lin(lin)
        return float(got.error), int(got.inlier)


def gate(case, idx, d2):
    """The kernel's inlier gate on the correspondences it reported, in float32 as the kernel applies it (a neighbour was found and
    d2 <= max_corr * max_corr); the rejected ones become what the generic tests hand in: d2 = 100. Nothing may sit near the gate."""
    mc = np.float32(case.max_corr)
    inl = (idx >= 0) & (d2 <= mc * mc)
    assert (d2[inl] < 0.25 * mc * mc).all() and ((idx[~inl] < 0) | (d2[~inl] > 4.0 * mc * mc)).all()
    return case.with_correspondences(np.where(inl, idx, 0), np.where(inl, d2, np.float32(f64.REJECTED_D2)))


def prepared_case(n):
    """make_case over the 3000-point target, every seventh source point moved 50 m away: no correspondence within max_corr."""
    case = f64.make_case(n, N_TARGET, seed=5000 + n, reject_every=0)
    far = np.arange(n) % 7 == 3
    case.src[far, 0] += 50.0
    return case, far


@pytest.fixture(scope="module")
def prepared_inputs(sp):
    """Per (factor, n): the case with the correspondences the fused kernel itself found (they do not depend on the loss: found once,
    with NONE), gated on the host, and the robust scale of those correspondences."""
    cache = {}

    def get(factor, n):
        if (factor, n) not in cache:
            case, far = prepared_case(n)
            got, idx, d2 = PreparedPath(sp, case, factor, "NONE").iteration_fused(1.0)
            found = gate(case, idx, d2)
            assert np.array_equal(found.inliers, ~far) and int(got.inlier) == int((~far).sum())
            cache[(factor, n)] = (found, f64.robust_scale(found, factor))
        return cache[(factor, n)]

    return get


def check_prepared(sp, orc, case, scale, factor, loss, path, tag, trials=TRIALS):
    ref64 = f64.system_fd(case, factor, loss, scale)
    oref = orc.gicp_linearize(*oracle_args(case, factor, loss, scale))
    got, idx, d2 = path.iteration_fused(scale)
    assert np.array_equal(gate(case, idx, d2).nn, case.nn), tag  # the same correspondences as the run that fixed the scale
    H, b, error, inlier = lin_result(got)
    hold(tag + " fused", H, b, error, inlier, ref64, oref)
    for twist in trials:
        T_trial = orc.isometry_mul(case.T, orc.se3_exp(twist))  # T <- T exp(delta), as a trial step makes it
        e, c = path.error_prepared(scale, T_trial)
        e64 = f64.error_f64(case, factor, loss, scale, T_trial)
        oe, oc = orc.gicp_error(case.src, case.scov, case.tgt, case.tcov, case.nrm, case.nn, case.d2, T_trial, case.max_corr, factor,
                                loss, scale)
        d64, dor = f64.relative(abs(e - e64), e64), f64.relative(abs(e - oe), e64)
        print(f"  K12 f64 {d64:.1e}  oracle {dor:.1e}", end="")
        assert c == oc == ref64["inlier"], tag
        assert d64 <= TOL_F64 and dor <= TOL_ORACLE, (tag, twist, d64, dor)
    return ref64, oref


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("loss", f64.LOSSES)
@pytest.mark.parametrize("factor", ["GICP", "POINT_TO_DISTRIBUTION"])
def test_prepared_and_fused_kernels_match_float64_and_oracle(sp, orc, prepared_inputs, factor, loss, n):
    case, scale = prepared_inputs(factor, n)
    check_prepared(sp, orc, case, scale, factor, loss, PreparedPath(sp, case, factor, loss), f"prepared n={n} {factor} {loss}")


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("factor", ["GICP", "POINT_TO_DISTRIBUTION"])
def test_tukey_on_every_form_of_the_prepared_kernels(sp, orc, prepared_inputs, factor, n):
    """TUKEY has the only hard zero branch and the only powf, and one instantiation per form: both searches of the fused iteration
    (fast_nn 0 / 1), and the linearisation step of sp_gicp_align_optimize with a wave per point and with a lane per point
    (sp_gicp_source_set_wave_per_point 2 / 0; a wave per point needs the fast search). One Gauss-Newton iteration of that launch
    reports the system of its only linearisation, at the initial pose."""
    case, scale = prepared_inputs(factor, n)
    for fast_nn in (0, 1):
        ref64, oref = check_prepared(sp, orc, case, scale, factor, "TUKEY", PreparedPath(sp, case, factor, "TUKEY", fast_nn),
                                     f"prepared n={n} {factor} TUKEY fast_nn={fast_nn}", trials=TRIALS[:1])
    assert (ref64["w"] == 0.0).sum() >= n // 5 and (ref64["w"] > 0.0).sum() >= n // 5  # both branches populated
    S = sp.PointCloudShared(dev(case.src), covs=dev(case.scov))
    prep = sp.PreparedTarget(sp.GridKNN.build(dev(case.tgt)), dev(case.tcov), reg_type=factor)
    p = sp.RegistrationParams(reg_type=factor, robust_type="TUKEY", robust_default_scale=scale, optimization_method="GN",
                              max_iterations=1, max_correspondence_distance=case.max_corr)
    for wave, fast_nn in ((2, 1), (0, 1), (0, 0)):
        reg = sp.Registration(p)
        reg._prepared_source(len(case.src))
        reg._set_source_option("fast_nn", fast_nn)
        sp.check(sp._lib.lib().sp_gicp_source_set_wave_per_point(reg._psrc._h, wave))
        res = reg.align_optimize(S, prep, case.T, [scale])
        assert res is not None, "the persistent launch must be available on an idle MI355X"
        assert res.linearizations == 1 and np.array_equal(res.T_lin, case.T)
        hold(f"optimiser n={n} {factor} TUKEY wave={wave} fast_nn={fast_nn}", res.H, res.b, res.error_raw, res.inlier, ref64, oref)
