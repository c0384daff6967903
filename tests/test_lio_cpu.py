"""The 15-DoF LiDAR-inertial alignment without a GPU (csrc/lio_host.hip through the C ABI and its api wrappers):

1. the ABI: every new name is declared, exported and in _lib.SIGNATURES, the ABI stays 7;
2. the reference's own tests (cpp/tests/test_imu_factor.cpp: twelve, cpp/tests/test_lio_registration.cpp: two) restated as
   known answers with the reference's tolerances (1e-5, 1e-6 for the algebraic identities), each through the C call and
   through the api wrapper;
3. every building block against the float64 model tests/f64_lio.py: error <= 4 K eps32 kappa scale over all entries and 8
   seeds. kappa = cond_inf of the matrix for what solves or inverts, 1 for products and sums; scale = the largest magnitude of
   the terms summed, or of the float64 answer for a solution; K = max(1, K_ref), K_ref the worst error / (eps32 kappa scale)
   of the SAME formulas run in numpy float32 (`kref` below; never measured on the library). `pytest -s` prints both;
4. the stepper with the ORACLE as the device (the pattern of tests/test_opt_stepper_cpu.py): brute-force neighbours + K11 for a
   linearisation, K12 for a trial. Every candidate state the stepper asks about is compared with the float64 model's under
   the bound of (3); a decision is compared only where the float64 margin exceeds the bound; structure is asserted exactly."""
import ctypes as C

import numpy as np
import pytest

import f64_lio as M
from test_gpu_optimize import inputs

EPS = M.EPS32
SEEDS = list(range(8))
METHOD = {"GN": 0, "LM": 1, "DOGLEG": 2}
NEW_SYMBOLS = ["sp_imu_manifold_residual_host", "sp_imu_hessian_gradient_host", "sp_imu_gradient_host", "sp_lio_add_icp_factor_host",
               "sp_lio_directional_weighting_host", "sp_lio_solve_ldlt_host", "sp_lio_retract_host",
               "sp_lio_imu_to_lidar_jacobian_host", "sp_lio_transform_covariance_host", "sp_dogleg_step_n_host",
               "sp_lio_stepper_create", "sp_lio_stepper_destroy", "sp_lio_stepper_next", "sp_lio_stepper_linearized",
               "sp_lio_stepper_trial", "sp_lio_stepper_result"]


@pytest.fixture(scope="module")
def sp():
    from sycl_points_amd import _lib

    _lib.build()
    import sycl_points_amd.api as api

    return api


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def cm(Mx):  # row-major numpy -> column-major floats
    return np.ascontiguousarray(np.asarray(Mx, np.float32).T).reshape(-1)


# ------------------------------------------------------------------------------------------------------------- 1. ABI
def test_abi_is_additive(sp):
    import os
    import re

    from sycl_points_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sycl_points_amd.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.lib().sp_abi_version() == 7
    # the 6-DoF entry point keeps its signature
    assert _lib.SIGNATURES["sp_dogleg_step_host"][1] == [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]


# --------------------------------------------------------------------------------------------- 2. the reference's known answers
def rot_z(a):
    c, s = np.float32(np.cos(np.float32(a))), np.float32(np.sin(np.float32(a)))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)


def hessian_gradient(sp, via, pred, op, P):
    if via == "api":
        return sp.compute_imu_hessian_gradient(pred, op, P)
    H, b, ok = np.full(225, 7, np.float32), np.full(15, 7, np.float32), C.c_int(-1)
    assert sp._lib.lib().sp_imu_hessian_gradient_host(vp(pred.pack()), vp(op.pack()), vp(cm(P)), vp(H), vp(b), C.byref(ok)) == 0
    return bool(ok.value), H.reshape(15, 15).T.copy(), b


def manifold_residual(sp, via, pred, op):
    if via == "api":
        return sp.compute_manifold_residual(pred, op)
    r = np.full(15, 7, np.float32)
    assert sp._lib.lib().sp_imu_manifold_residual_host(vp(pred.pack()), vp(op.pack()), vp(r)) == 0
    return r


def imu_gradient(sp, via, pred, op, H):
    if via == "api":
        return sp.compute_imu_gradient(pred, op, H)
    b = np.full(15, 7, np.float32)
    assert sp._lib.lib().sp_imu_gradient_host(vp(pred.pack()), vp(op.pack()), vp(cm(H)), vp(b)) == 0
    return b


def directional_weighting(sp, via, H, b, inlier, prm):
    if via == "api":
        f = sp.LIOLinearizedResult(H=H.copy(), b=b.copy(), inlier=inlier)
        sp.apply_directional_icp_weighting(f, sp.DirectionalIcpWeightingParams(*prm))
        return f.H, f.b
    c = sp._lib.LioLinearized()
    C.memmove(c.H, cm(H).ctypes.data, 900)
    C.memmove(c.b, np.asarray(b, np.float32).ctypes.data, 60)
    c.inlier = inlier
    p = sp._lib.LioDirectionalParams(int(prm[0]), *prm[1:])
    assert sp._lib.lib().sp_lio_directional_weighting_host(C.byref(c), C.byref(p)) == 0
    return np.array(c.H, np.float32).reshape(15, 15).T.copy(), np.array(c.b, np.float32)


def diag_cov(s):
    return (np.float32(s) * np.eye(15, dtype=np.float32)).astype(np.float32)


def is_approx(a, b, prec):  # Eigen's isApprox: |a - b| <= prec min(|a|, |b|) in the Frobenius norm
    return np.linalg.norm(a - b) <= prec * min(np.linalg.norm(a), np.linalg.norm(b))


def is_zero(a, prec=1e-6):  # Eigen's isZero(prec) of a vector / matrix: every |entry| <= prec
    return bool(np.all(np.abs(a) <= prec))


VIA = ["c", "api"]


@pytest.mark.parametrize("via", VIA)
def test_known_answers_of_test_imu_factor(sp, via):
    S = sp.IMUState
    v3 = lambda *x: np.array(x, np.float32)  # noqa: E731
    hg = lambda pred, op, P: hessian_gradient(sp, via, pred, op, P)  # noqa: E731
    # 1 HessianIsInverseOfCovariance
    ok, H, b = hg(S(), S(), diag_cov(0.04))
    assert ok and is_approx(H @ diag_cov(0.04), np.eye(15, dtype=np.float32), 1e-6)
    # 2 ZeroResidualGivesZeroGradient
    ok, H, b = hg(S(), S(), diag_cov(0.01))
    assert ok and is_zero(b)
    # 3 PositionResidualOnlyAffectsPositionBlock
    ok, H, b = hg(S(), S(position=v3(1, 2, 3)), diag_cov(0.25))
    assert ok and np.abs(b[:3] - 4.0 * v3(1, 2, 3)).max() <= 1e-5 and is_zero(b[3:])
    # 4 VelocityResidualOnly
    ok, H, b = hg(S(), S(velocity=v3(0.5, -1.0, 0.0)), diag_cov(1.0))
    assert ok and np.abs(b[6:9] - v3(0.5, -1.0, 0.0)).max() <= 1e-5 and is_zero(b[:6]) and is_zero(b[9:])
    # 5 BiasResiduals
    ok, H, b = hg(S(), S(accel_bias=v3(0.1, 0.2, 0.3), gyro_bias=v3(0.4, 0.5, 0.6)), diag_cov(2.0))
    assert ok and np.abs(b[9:] - 0.5 * v3(0.1, 0.2, 0.3, 0.4, 0.5, 0.6)).max() <= 1e-5 and is_zero(b[:9])
    # 6 RotationResidualSO3Log
    angle = np.float32(np.pi) / np.float32(6)
    ok, H, b = hg(S(), S(rotation=rot_z(angle)), diag_cov(1.0))
    assert ok and np.abs(b[3:6] - v3(0, 0, angle)).max() <= 1e-5 and is_zero(b[:3]) and is_zero(b[6:])
    # 7 RotationResidualAntisymmetry
    xa, xb = S(), S(rotation=rot_z(np.float32(np.pi) / np.float32(4)))
    _, _, bab = hg(xa, xb, diag_cov(1.0))
    _, _, bba = hg(xb, xa, diag_cov(1.0))
    assert is_approx(bab[3:6], -bba[3:6], 1e-5)
    # 8 HessianIsSymmetricPositiveDefinite
    P = diag_cov(0.1)
    P[0, 1] = P[1, 0] = 0.005
    P[6, 7] = P[7, 6] = 0.003
    ok, H, b = hg(S(), S(position=v3(1.0, -0.5, 0.2), velocity=v3(0.3, 0.1, -0.4), gyro_bias=v3(0.01, -0.02, 0.005)), P)
    assert ok and is_approx(H, H.T, 1e-6)
    np.linalg.cholesky(H.astype(np.float64))  # raises unless positive definite
    # 9 GradientEqualsHTimesResidual
    xo = S(position=v3(0.3, -0.1, 0.5), rotation=rot_z(0.2), velocity=v3(-0.2, 0.4, 0.0), accel_bias=v3(0.01, -0.02, 0.03),
           gyro_bias=v3(0.005, 0.003, -0.001))
    ok, H, b = hg(S(), xo, diag_cov(0.05))
    r = manifold_residual(sp, via, S(), xo)
    assert ok and is_approx(b, (H @ r).astype(np.float32), 1e-6)
    assert is_approx(imu_gradient(sp, via, S(), xo, H), b, 1e-6)
    # 10 NearIdentityRotationIsNumericallyStable
    ok, H, b = hg(S(), S(rotation=rot_z(1e-8)), diag_cov(1.0))
    assert ok and np.all(np.isfinite(b)) and np.linalg.norm(b[3:6]) <= 1e-5
    # 11 StateIndexConstantsAreCorrect
    assert (S.kIdxPos, S.kIdxRot, S.kIdxVel, S.kIdxAccBias, S.kIdxGyrBias, S.kDOF) == (0, 3, 6, 9, 12, 15)
    # 12 IllConditionedCovarianceReturnsZero
    ok, H, b = hg(S(), S(position=v3(1, 2, 3)), np.zeros((15, 15), np.float32))
    assert not ok and not H.any() and not b.any()


@pytest.mark.parametrize("via", VIA)
def test_known_answers_of_test_lio_registration(sp, via):
    # DirectionalIcpWeightingAttenuatesWeakDirections
    H, b = np.zeros((15, 15), np.float32), np.zeros(15, np.float32)
    H[0, 0], H[1, 1], H[3, 3] = 1.0, 20.0, 1.0
    b[0], b[1], b[3] = 10.0, 20.0, 10.0
    H2, b2 = directional_weighting(sp, via, H, b, 100, (True, 0.05, 0.05, 0.1, 0.25))
    for got, want in ((H2[0, 0], 0.2), (b2[0], 2.0), (H2[1, 1], 20.0), (b2[1], 20.0), (H2[3, 3], 0.25), (b2[3], 2.5)):
        assert abs(got - want) <= 1e-5, (got, want)
    # DirectionalIcpWeightingPreservesCoupledFactorStructure
    H, b = np.zeros((15, 15), np.float32), np.zeros(15, np.float32)
    H[0, 0] = H[3, 3] = 1.0
    H[0, 3] = H[3, 0] = 0.5
    H2, b2 = directional_weighting(sp, via, H, b, 100, (True, 0.1, 0.1, 0.1, 0.4))
    for got, want in ((H2[0, 0], 0.1), (H2[3, 3], 0.4), (H2[0, 3], 0.1), (H2[3, 0], 0.1)):
        assert abs(got - want) <= 1e-5, (got, want)
    Hp = H2[:6, :6]
    assert is_approx(Hp, Hp.T, 1e-5) and np.linalg.eigvalsh(Hp.astype(np.float64)).min() >= -1e-5


# ------------------------------------------------------------------------------------ 3. building blocks against float64
@pytest.fixture(scope="module")
def clouds(orc):
    src, scov, tgt, tcov, T_gt = inputs(orc, 900, 8.0)
    return dict(src=src, scov=scov, tgt=tgt, tcov=tcov, T_gt=T_gt, tnrm=orc.normals_from_cov(tgt, tcov))


def oracle_lin(orc, cl, T, reg="GICP", loss="NONE", scale=10.0):
    nn = orc.knn_bruteforce(orc.transform_points(cl["src"], T), cl["tgt"], 1)
    nrm = cl["tnrm"] if reg == "POINT_TO_PLANE" else None
    return orc.gicp_linearize(cl["src"], cl["scov"], cl["tgt"], cl["tcov"], nrm, nn[0], nn[1], T, 2.0, reg, loss, scale), nn


def random_rotation(rs, lo, hi):
    axis = rs.normal(size=3)
    return M.rodrigues(axis / np.linalg.norm(axis) * rs.uniform(lo, hi))


def cond_inf(A):
    A = np.asarray(A, np.float64)
    return float(np.linalg.norm(A, np.inf) * np.linalg.norm(np.linalg.inv(A), np.inf))


def make_case(orc, cl, seed):
    """One seed's inputs, all float32: a state 1-3 cm / 0.5-1 degree off the truth, the oracle's K11 sums there, a random SPD prior
    scaled to the ICP information, a predicted state nearby, non-identity extrinsics with a 10-30 cm lever arm."""
    rs = np.random.RandomState(1000 + seed)
    T_gt = np.asarray(cl["T_gt"], np.float64)
    d = rs.normal(size=3)
    off = np.eye(4)
    off[:3, :3] = random_rotation(rs, np.deg2rad(0.5), np.deg2rad(1.0))
    off[:3, 3] = d / np.linalg.norm(d) * rs.uniform(0.01, 0.03)
    T = (T_gt @ off).astype(np.float32)
    lin, _ = oracle_lin(orc, cl, T)
    f = np.float32
    op = M.St(T[:3, 3], T[:3, :3], rs.uniform(-1, 1, 3), rs.uniform(-0.1, 0.1, 3), rs.uniform(-0.01, 0.01, 3), f)
    pred = M.St(op.p + rs.uniform(-0.02, 0.02, 3).astype(f), (op.R.astype(np.float64) @ random_rotation(rs, 0.002, 0.01)).astype(f),
                op.v + rs.uniform(-0.05, 0.05, 3).astype(f), op.ba + rs.uniform(-0.01, 0.01, 3).astype(f),
                op.bg + rs.uniform(-0.001, 0.001, 3).astype(f), f)
    w = M.icp_weight(lin["error"], lin["inlier"], 3)
    Hi, _ = M.add_icp(np.zeros((15, 15)), np.zeros(15), lin["H"].astype(np.float64), lin["b"].astype(np.float64),
                      op.R.astype(np.float64), w)
    h = np.mean(np.diag(Hi)[:6])
    Q, _ = np.linalg.qr(rs.normal(size=(15, 15)))
    P = ((Q * rs.uniform(1.0, 4.0, 15)) @ Q.T / h)
    P = ((P + P.T) / 2).astype(f)
    T_ext = np.eye(4)
    T_ext[:3, :3] = random_rotation(rs, 0.1, 0.6)
    lever = rs.normal(size=3)
    T_ext[:3, 3] = lever / np.linalg.norm(lever) * rs.uniform(0.10, 0.30)
    return dict(rs=rs, lin=lin, op=op, pred=pred, P=P, w=f(w), T_ext=T_ext.astype(f), delta=(rs.normal(size=15) * 0.02).astype(f))


def up(x, dt):
    return M.St(x.p, x.R, x.v, x.ba, x.bg, dt)


def model_quantities(c, dt, radius_for=None):
    """Every checked quantity of one seed from the model in precision dt, on the float32 inputs of `c`. Each entry: value, kappa,
    scale (kappa and scale are taken from the float64 run)."""
    lin, op, pred, P = c["lin"], up(c["op"], dt), up(c["pred"], dt), c["P"].astype(dt)
    H6, b6, w = lin["H"].astype(dt), lin["b"].astype(dt), dt(c["w"])
    out = {}
    He, be = M.add_icp(np.zeros((15, 15), dt), np.zeros(15, dt), H6, b6, op.R, w)
    out["embed_H"] = (He, 1.0, float(w) * np.abs(H6).max())
    out["embed_b"] = (be, 1.0, float(w) * np.abs(b6).max())
    # a threshold between the block's eigenvalues (branch safety is asserted by the caller from c["dirw_eigs"])
    Hf, bf, eigs = M.directional(He, be, int(lin["inlier"]), *c["dirw"])
    out["filter_H"] = (Hf, 1.0, np.abs(He).max())
    out["filter_b"] = (bf, 1.0, np.abs(be).max())
    c.setdefault("dirw_eigs", eigs)
    r = M.residual(pred, op)
    out["residual"] = (r, 1.0, max(1.0, np.abs(op.pack()).max(), np.abs(pred.pack()).max()))
    Hi, bi = M.imu_hessian_gradient(pred, op, P)
    out["H_imu"] = (Hi, cond_inf(c["P"]), np.abs(Hi).max())
    out["b_imu"] = (bi, cond_inf(c["P"]), np.abs(bi).max())
    Hc = (Hf + Hi).astype(dt)
    bc = (bf + bi).astype(dt)
    c.setdefault("Hc32", Hc.astype(np.float32))
    c.setdefault("bc32", bc.astype(np.float32))
    Hs, bs = c["Hc32"].astype(dt), c["bc32"].astype(dt)  # the float32 system every implementation solves
    delta, Ppost = M.solve(Hs, bs)
    out["delta"] = (delta, cond_inf(c["Hc32"]), np.abs(delta).max())
    out["P_post"] = (Ppost, cond_inf(c["Hc32"]), np.abs(Ppost).max())
    x2 = M.retract(op, c["delta"].astype(dt))
    out["retract"] = (x2.pack(), 1.0, max(1.0, np.abs(op.pack()).max()))
    T_ext = c["T_ext"].astype(dt)
    J = M.jacobian(T_ext, op.R)
    out["jacobian"] = (J, 1.0, max(1.0, np.abs(J).max()))
    Pl = M.transform_covariance(P, T_ext, op.R, 0)
    terms = np.abs(J).max() ** 2 * np.abs(P).max()
    out["cov_imu_to_lidar"] = (Pl, 1.0, float(terms))
    c.setdefault("Pl32", Pl.astype(np.float32))
    Pb = M.transform_covariance(c["Pl32"].astype(dt), T_ext, op.R, 1)
    Ji = M.jacobian(T_ext, op.R, inverse=True)
    out["cov_lidar_to_imu"] = (Pb, 1.0, float(np.abs(Ji).max() ** 2 * np.abs(c["Pl32"]).max()))
    # the round trip lidar_to_imu(imu_to_lidar(P)) = P: each implementation is fed its OWN first product
    out["round_trip"] = (M.transform_covariance(Pl, T_ext, op.R, 1), 1.0, float(np.abs(Ji).max() ** 2 * np.abs(Pl).max()))
    return out


def library_quantities(sp, c):
    S = sp.IMUState
    to_api = lambda x: S.unpack(x.pack().astype(np.float32))  # noqa: E731
    op, pred, lin = to_api(c["op"]), to_api(c["pred"]), c["lin"]
    out = {}
    f = sp.LIOLinearizedResult()
    sp.add_icp_factor(f, lin, op.rotation, float(c["w"]))
    out["embed_H"], out["embed_b"] = f.H.copy(), f.b.copy()
    assert f.inlier == lin["inlier"] and f.error_icp == np.float32(c["w"] * np.float32(lin["error"]))
    sp.apply_directional_icp_weighting(f, sp.DirectionalIcpWeightingParams(*c["dirw"]))
    out["filter_H"], out["filter_b"] = f.H, f.b
    out["residual"] = sp.compute_manifold_residual(pred, op)
    ok, out["H_imu"], out["b_imu"] = sp.compute_imu_hessian_gradient(pred, op, c["P"])
    assert ok
    ok, out["delta"], out["P_post"] = sp.solve_ldlt(c["Hc32"], c["bc32"], want_posterior=True)
    assert ok
    out["retract"] = sp.retract(op, c["delta"]).pack()
    out["jacobian"] = sp.imu_to_lidar_jacobian(c["T_ext"], op.rotation)
    out["cov_imu_to_lidar"] = sp.transform_covariance_imu_to_lidar(c["P"], c["T_ext"], op.rotation)
    out["cov_lidar_to_imu"] = sp.transform_covariance_lidar_to_imu(c["Pl32"], c["T_ext"], op.rotation)
    out["round_trip"] = sp.transform_covariance_lidar_to_imu(out["cov_imu_to_lidar"], c["T_ext"], op.rotation)
    return out


def dirw_for(c, rs):
    """Directional-weighting thresholds between the eigenvalues of this seed's blocks, every eigenvalue at least 1 % away from
    min_info and from 0: the weakest translation direction is weak, the others strong; for the rotation block the two weakest."""
    lin, op = c["lin"], up(c["op"], np.float64)
    He, _ = M.add_icp(np.zeros((15, 15)), np.zeros(15), lin["H"].astype(np.float64), lin["b"].astype(np.float64), op.R, float(c["w"]))
    lt = np.linalg.eigvalsh(He[:3, :3])
    lr = np.linalg.eigvalsh(He[3:6, 3:6])
    n = lin["inlier"]
    return (True, float(np.sqrt(lt[0] * lt[1]) / n), float(np.sqrt(lr[1] * lr[2]) / n), 0.2, 0.3)


@pytest.fixture(scope="module")
def cases(orc, clouds):
    out = []
    for seed in SEEDS:
        c = make_case(orc, clouds, seed)
        c["dirw"] = dirw_for(c, c["rs"])
        c["f64"] = model_quantities(c, np.float64)
        out.append(c)
    return out


@pytest.fixture(scope="module")
def kref(cases):
    """K_ref per quantity: the worst error / (eps32 kappa scale) of the model's formulas run in numpy float32, over all seeds."""
    K = {}
    for c in cases:
        f32 = model_quantities(c, np.float32)
        for name, (want, kappa, scale) in c["f64"].items():
            err = np.abs(np.asarray(f32[name][0], np.float64) - want).max()
            K[name] = max(K.get(name, 0.0), err / (EPS * kappa * scale))
    return K


def test_building_blocks_against_float64(sp, cases, kref):
    worst = {}
    for c in cases:
        for (lam, min_info) in c["dirw_eigs"]:  # branch safety
            assert min_info > 0 and np.all(np.abs(lam / min_info - 1.0) >= 0.01) and np.all(lam >= 0.01 * min_info)
            assert (lam < min_info).any() and (lam > min_info).any()  # both kinds of direction occur
        assert cond_inf(c["P"]) <= 1e3 and cond_inf(c["Hc32"]) <= 1e3, (cond_inf(c["P"]), cond_inf(c["Hc32"]))
        lever = np.linalg.norm(c["T_ext"][:3, 3])
        assert 0.10 <= lever <= 0.30 and not np.allclose(c["T_ext"][:3, :3], np.eye(3), atol=0.05)
        got = library_quantities(sp, c)
        for name, (want, kappa, scale) in c["f64"].items():
            err = np.abs(np.asarray(got[name], np.float64) - want).max()
            worst[name] = max(worst.get(name, 0.0), err / (EPS * kappa * scale))
        # the model's round trip is P as far as the float32 extrinsic rotation is orthonormal (J^-1 is the analytic inverse)
        assert np.abs(c["f64"]["round_trip"][0] - c["P"]).max() <= EPS * np.abs(c["P"]).max()
    print("\n[lio-f64] worst error / (eps32 kappa scale): quantity, numpy float32 (K_ref), library")
    for name in worst:
        print(f"[lio-f64]   {name:18s} {kref.get(name, float('nan')):8.3f} {worst[name]:8.3f}")
    for name, k in kref.items():
        assert worst[name] <= 4 * max(1.0, k), (name, worst[name], k)


def test_directional_weighting_exact_cases(sp, cases):
    c = cases[0]
    f = sp.LIOLinearizedResult()
    sp.add_icp_factor(f, c["lin"], c["op"].R, 1.0)
    H0, b0 = f.H.copy(), f.b.copy()
    # disabled, and inlier == 0: untouched, bit for bit
    sp.apply_directional_icp_weighting(f, sp.DirectionalIcpWeightingParams(False, 1e9, 1e9, 0.0, 0.0))
    assert np.array_equal(f.H, H0) and np.array_equal(f.b, b0)
    g = sp.LIOLinearizedResult(H=H0.copy(), b=b0.copy(), inlier=0)
    sp.apply_directional_icp_weighting(g, sp.DirectionalIcpWeightingParams(True, 1e9, 1e9, 0.0, 0.0))
    assert np.array_equal(g.H, H0) and np.array_equal(g.b, b0)
    # an eigenvalue <= 0 is removed whatever the weak scale: a block with an exact null direction
    H = np.zeros((15, 15), np.float32)
    H[0, 0], H[1, 1], H[2, 2], H[3, 3], H[4, 4], H[5, 5] = 2.0, 3.0, 0.0, 1.0, 1.0, -1.0
    b = np.ones(15, np.float32)
    k = sp.LIOLinearizedResult(H=H, b=b, inlier=10)
    sp.apply_directional_icp_weighting(k, sp.DirectionalIcpWeightingParams(True, 0.0, 0.0, 1.0, 1.0))
    assert np.allclose(np.diag(k.H)[:6], [2, 3, 0, 1, 1, 0], atol=1e-6) and np.allclose(k.b[:6], [1, 1, 0, 1, 1, 0], atol=1e-6)
    assert np.array_equal(k.b[6:], b[6:])


def draw_dogleg(rs, n, branch):
    """H, g, radius whose float64 dog-leg takes `branch`, the deciding norms at least 1 % from the radius."""
    for _ in range(1000):
        Q, _ = np.linalg.qr(rs.normal(size=(n, n)))
        lam = rs.uniform(1.0, 50.0, n)
        if branch == 3:
            lam[0] = -lam[0]  # indefinite: no Gauss-Newton point
        H = (Q * lam) @ Q.T
        H = ((H + H.T) / 2).astype(np.float32)
        g = rs.normal(size=n).astype(np.float32)
        H64, g64 = H.astype(np.float64), g.astype(np.float64)
        _, _, _, _, n_gn, n_sd = M.dogleg(H64, g64, 1.0)
        radius = {0: 1.5 * n_gn, 1: 0.5 * n_sd, 2: 0.5 * (n_sd + n_gn), 3: 2.0 * n_sd}[branch]
        p, norm, pred, br, n_gn, n_sd = M.dogleg(H64, g64, radius)
        far = all(abs(x / radius - 1.0) >= 0.01 for x in (n_gn, n_sd) if x > 0)
        if br == branch and far:
            return H, g, np.float32(radius)
    raise AssertionError("no draw")


@pytest.mark.parametrize("n", [6, 15])
def test_dogleg_step_against_float64(sp, n):
    rs = np.random.RandomState(77 + n)
    seen, worst, kworst = set(), 0.0, 0.0
    for branch in (0, 1, 2, 3):
        for _ in range(8):
            H, g, radius = draw_dogleg(rs, n, branch)
            H64, g64 = H.astype(np.float64), g.astype(np.float64)
            p64, norm64, pred64, br, _, _ = M.dogleg(H64, g64, float(radius))
            p32, norm32, pred32, br32, _, _ = M.dogleg(H, g, radius)
            seen.add(br)
            kappa = cond_inf(H64) if br in (0, 2) else 1.0
            scale = np.abs(p64).max()
            p, norm, pred = sp.compute_dogleg_step(H, g, float(radius))
            kref = np.abs(p32.astype(np.float64) - p64).max() / (EPS * kappa * scale) if br32 == br else 0.0
            err = np.abs(p.astype(np.float64) - p64).max() / (EPS * kappa * scale)
            worst, kworst = max(worst, err), max(kworst, kref)
            assert err <= 4 * max(1.0, kref), (n, branch, err, kref)
            assert abs(norm - norm64) <= 4 * max(1.0, kref) * EPS * kappa * max(norm64, float(radius))
            terms = np.abs(g64) @ np.abs(p64) + 0.5 * np.abs(p64) @ np.abs(H64) @ np.abs(p64)
            assert abs(pred - pred64) <= 4 * max(1.0, kref) * EPS * kappa * terms
            if n == 6:  # the arithmetic of the 6-DoF entry point, bit for bit
                p6, n6, r6 = np.zeros(6, np.float32), C.c_float(), C.c_float()
                sp._lib.lib().sp_dogleg_step_host(vp(np.ascontiguousarray(H)), vp(g), C.c_float(radius), vp(p6), C.byref(n6), C.byref(r6))
                assert np.array_equal(p6, p) and n6.value == norm and r6.value == pred
    assert seen == {0, 1, 2, 3}
    print(f"\n[lio-f64] dog-leg n={n}: worst error / (eps32 kappa scale): numpy float32 {kworst:.3f}, library {worst:.3f}")
    bad = C.c_float()
    assert sp._lib.lib().sp_dogleg_step_n_host(7, vp(H), vp(g), C.c_float(1.0), vp(np.zeros(15, np.float32)), C.byref(bad),
                                               C.byref(bad)) == sp._lib.SP_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------ 4. the stepper, the oracle as the device
def lio_params(sp, method, total, **kw):
    opt = sp.RegistrationParams(optimization_method=method, **{k: v for k, v in kw.items()
                                                               if hasattr(sp.RegistrationParams(), k) and not k.startswith("criteria_")})
    p = sp.LIORegistrationParams(total_iterations=total, optimization=opt)
    for k, v in kw.items():
        if k in ("criteria_rotation", "criteria_translation"):
            setattr(p.criteria, k[len("criteria_"):], v)
        elif hasattr(p.robust, k):
            setattr(p.robust, k, v)
        elif hasattr(p.directional_icp_weighting, k):
            setattr(p.directional_icp_weighting, k, v)
        elif k == "invalid_regularization_factor":
            p.invalid_regularization_factor = v
    return p


def drive(sp, params, factor, pred, P, P_prev, update_bias, linearize, trial, watch=None):
    """The ask-and-serve loop. linearize(req) -> Linearized-like dict, trial(req) -> (error, inlier); watch(req, answer) sees every
    request with what was served. Returns (requests, LioResult)."""
    lib, L = sp._lib, sp._lib.lib()
    prm, facts = params.c_struct(), sp.lio_factor_facts(factor)
    h, res, reqs = C.c_void_p(), lib.LioResult(), []
    sp.check(L.sp_lio_stepper_create(C.byref(prm), C.byref(facts), vp(pred.pack()), vp(cm(P)), vp(cm(P_prev)), int(update_bias),
                                     C.byref(h)))
    try:
        while True:
            req = lib.LioRequest()
            sp.check(L.sp_lio_stepper_next(h, C.byref(req)))
            reqs.append(req)
            if req.want == lib.OPT_WANT_DONE:
                if watch:
                    watch(req, None)
                break
            if req.want == lib.OPT_WANT_LINEARIZE:
                ans = linearize(req)
                assert L.sp_lio_stepper_trial(h, C.c_float(1.0), 1) == lib.SP_ERR_INVALID_ARGUMENT  # the wrong kind of answer ...
                again = lib.LioRequest()
                sp.check(L.sp_lio_stepper_next(h, C.byref(again)))
                assert bytes(again) == bytes(req)  # ... changes nothing
                sp.check(L.sp_lio_stepper_linearized(h, C.byref(sp._lin6(ans))))
            else:
                ans = trial(req)
                assert L.sp_lio_stepper_linearized(h, C.byref(lib.Linearized())) == lib.SP_ERR_INVALID_ARGUMENT
                again = lib.LioRequest()
                sp.check(L.sp_lio_stepper_next(h, C.byref(again)))
                assert bytes(again) == bytes(req)
                sp.check(L.sp_lio_stepper_trial(h, C.c_float(ans[0]), ans[1]))
            if watch:
                watch(req, ans)
        sp.check(L.sp_lio_stepper_result(h, C.byref(res)))
        assert L.sp_lio_stepper_linearized(h, C.byref(lib.Linearized())) == lib.SP_ERR_INVALID_ARGUMENT  # nothing is wanted once done
        assert L.sp_lio_stepper_trial(h, C.c_float(0.0), 0) == lib.SP_ERR_INVALID_ARGUMENT
    finally:
        L.sp_lio_stepper_destroy(h)
    return reqs, res


class OracleDevice:
    def __init__(self, orc, cl, reg, loss="NONE"):
        self.orc, self.cl, self.reg, self.loss, self.nn, self.T_lin = orc, cl, reg, loss, None, None

    def pose(self, req):
        return np.array(req.T, np.float32).reshape(4, 4).T

    def linearize(self, req):
        lin, self.nn = oracle_lin(self.orc, self.cl, self.pose(req), self.reg, self.loss, req.robust_scale)
        self.T_lin = np.array(req.T, np.float32)
        return lin

    def trial(self, req):
        assert np.array_equal(np.array(req.T_lin, np.float32), self.T_lin)  # the frozen correspondences are the latest ones
        cl = self.cl
        nrm = cl["tnrm"] if self.reg == "POINT_TO_PLANE" else None
        return self.orc.gicp_error(cl["src"], cl["scov"], cl["tgt"], cl["tcov"], nrm, self.nn[0], self.nn[1], self.pose(req), 2.0,
                                   self.reg, self.loss, req.robust_scale)


def start(cl, seed=0, scale=1.0):
    """Predicted state: the truth moved by a few centimetres / a degree, some velocity and biases; a valid SPD prior whose
    information is comparable to the ICP's; a previous posterior that is recognisable."""
    rs = np.random.RandomState(50 + seed)
    T = np.asarray(cl["T_gt"], np.float64) @ np.block([[M.rodrigues(np.array([0.01, -0.005, 0.02])), np.array([[0.05], [-0.04], [0.03]])],
                                                       [np.zeros((1, 3)), np.ones((1, 1))]])
    f = np.float32
    pred = M.St(T[:3, 3], T[:3, :3], [0.3, -0.2, 0.1], [0.02, -0.01, 0.03], [0.001, 0.002, -0.001], f)
    Q, _ = np.linalg.qr(rs.normal(size=(15, 15)))
    P = (Q * rs.uniform(1.0, 4.0, 15)) @ Q.T * scale
    P = ((P + P.T) / 2).astype(f)
    return pred, P, (np.eye(15) * 0.125).astype(f)


def api_state(sp, x):
    return sp.IMUState.unpack(np.asarray(x.pack(), np.float32))


CASES = [(m, r) for m in ("GN", "LM", "DOGLEG") for r in ("GICP", "POINT_TO_PLANE")]


@pytest.mark.parametrize("method,reg", CASES, ids=[f"{m}-{r}" for m, r in CASES])
def test_stepper_against_float64_with_the_oracle_as_device(sp, orc, clouds, kref, method, reg):
    f64 = np.float64
    factor = sp.RegistrationParams(reg_type=reg)
    dim = 1 if reg == "POINT_TO_PLANE" else 3
    pred32, P, P_prev = start(clouds, scale=1e-3 if reg == "GICP" else 1e-2)
    params = lio_params(sp, method, 6, gn_lambda=1e-3)
    o = params.optimization
    dirw = (True, 10.0, 10.0, 0.2, 0.2)
    dev = OracleDevice(orc, clouds, reg)
    pred = up(pred32, f64)
    H_imu = np.linalg.inv(P.astype(f64))
    K, K_retract, K_post = max(1.0, kref["delta"]), max(1.0, kref["retract"]), max(1.0, kref["P_post"])  # what is solved: delta's K
    S = dict(n_lin=0, steps=0, skipped=0, expect=None, phase=None, worst=0.0)

    def state_bound(kappa, delta, x):
        return 4 * EPS * (K * kappa * np.abs(delta).max() + K_retract * max(1.0, np.abs(x.pack()).max()))  # delta, then its retraction

    def cost_bound(x, e, w):
        r = M.residual(pred, x)
        return 4 * K * EPS * (abs(w * e) + 0.5 * np.abs(r) @ np.abs(H_imu) @ np.abs(r))

    def candidate(H, b, damping):
        if method == "DOGLEG":
            p, norm, _, br, _, _ = M.dogleg(H, b, damping)
            return M.freeze(p, True), cond_inf(H) if br in (0, 2) else 1.0, norm
        Hd = H + damping * np.eye(15)
        return -np.linalg.solve(Hd, b), cond_inf(Hd), None

    def check_state(req, want, bound, what):
        err = np.abs(np.array(req.state, f64) - want.pack()).max()
        S["worst"] = max(S["worst"], err / bound)
        assert err <= bound, (what, err, bound)

    def f32clamp(v, lo, hi):
        return np.float32(min(max(np.float32(v), np.float32(lo)), np.float32(hi)))

    def check_convergence(req, d, bound):
        """after an accepted step delta: converged (both norms under the criteria) leaves the level - with one level, the loop"""
        nr, nt = np.linalg.norm(d[3:6]), np.linalg.norm(d[0:3])
        slack = np.sqrt(3.0) * bound
        last = S["iteration"] + 1 >= 6
        if abs(nr - params.criteria.rotation) <= slack or abs(nt - params.criteria.translation) <= slack:
            S["skipped"] += 1
        elif not last:
            converged = nr < params.criteria.rotation and nt < params.criteria.translation
            assert (req.want == sp._lib.OPT_WANT_DONE) == converged, ("convergence", nr, nt)

    def watch(req, ans):
        lib = sp._lib
        x = M.St.unpack(np.array(req.state, np.float32), f64)
        e = S["expect"]
        if e is not None:  # what the float64 model said this request would be about
            kind, want, bound, decided = e
            if kind == "accept-or-not":
                # accepted: the loop goes on at the trial state, bit for bit; rejected: at the state of the linearisation
                accepted = req.want != lib.OPT_WANT_TRIAL and np.array_equal(np.array(req.state, np.float32), S["trial_state"])
                if not accepted and req.want != lib.OPT_WANT_TRIAL:
                    assert np.array_equal(np.array(req.state, np.float32), S["op"].pack().astype(np.float32))
                if decided is not None:
                    assert accepted == decided, ("decision", req.level, req.iteration)
                else:
                    S["skipped"] += 1
                if method == "LM" and req.want == lib.OPT_WANT_TRIAL:  # the next trial: the model's step at lambda * factor
                    w_state, w_bound, lam = S["after_reject"]
                    assert req.damping == lam
                    check_state(req, w_state, w_bound, "lm-next-trial")
                    S["trial_delta"], S["trial_delta_bound"] = S["delta_if_rejected"]
                if req.want == lib.OPT_WANT_LINEARIZE and req.level == S["level"]:  # the damping the step leaves behind
                    after = S["damping_after"][accepted]
                    if after is not None:
                        assert req.damping == after, (req.damping, after, accepted)
                    else:
                        S["skipped"] += 1
                if accepted:
                    check_convergence(req, S["trial_delta"], S["trial_delta_bound"])
            elif want is not None:
                check_state(req, want, bound, kind)
                if kind == "gn-next-state":
                    check_convergence(req, S["trial_delta"], S["trial_delta_bound"])
            S["expect"] = None
        if req.want == lib.OPT_WANT_DONE:
            return
        S["steps"] += 1
        if req.want == lib.OPT_WANT_LINEARIZE:
            H, b, w = M.combined_system(ans, x, pred, H_imu, True, S["n_lin"] == 0, dim, dirw, 1e4)
            S.update(n_lin=S["n_lin"] + 1, H=H, b=b, w=w, op=x, lin=ans, phase="lin", level=req.level, iteration=req.iteration)
            if method == "GN":
                d, kappa, _ = candidate(H, b, req.damping)
                S["expect"] = ("gn-next-state", M.retract(x, d), state_bound(kappa, d, x), None)
                S["trial_delta"], S["trial_delta_bound"] = d, 4 * K * EPS * kappa * np.abs(d).max()
            return
        # a trial
        if S["phase"] == "lin":  # the first trial of the outer iteration: at the operating state, bit for bit
            assert np.array_equal(np.array(req.T, np.float32), np.array(req.T_lin, np.float32))
            assert np.array_equal(np.array(req.state, np.float32), S["op"].pack().astype(np.float32))
            assert req.icp_weight == np.float32(S["w"]) or abs(req.icp_weight - S["w"]) <= 4 * EPS * S["w"]
            S["current"] = S["w"] * ans[0] + M.imu_cost(pred, x, H_imu)
            S["current_bound"] = cost_bound(x, ans[0], S["w"])
            S["phase"] = "candidate"
            d, kappa, norm = candidate(S["H"], S["b"], req.damping)
            S["expect"] = ("candidate-state", M.retract(S["op"], d), state_bound(kappa, d, S["op"]), None)
            S["trial_delta"], S["trial_delta_bound"], S["step_norm"] = d, 4 * K * EPS * kappa * np.abs(d).max(), norm
            return
        cost = S["w"] * ans[0] + M.imu_cost(pred, x, H_imu)
        margin = abs(cost - S["current"]) - (cost_bound(x, ans[0], S["w"]) + S["current_bound"])
        if method == "LM":
            decided = (cost <= S["current"]) if margin > 0 else None
            lam = np.float32(min(max(np.float32(req.damping) * np.float32(o.lm_lambda_factor), np.float32(o.lm_min_lambda)),
                                 np.float32(o.lm_max_lambda)))
            d, kappa, _ = candidate(S["H"], S["b"], float(lam))
            # accepted: the next request linearises at this very state; rejected: the next trial is the model's step at lambda * factor
            S["expect"] = ("accept-or-not", None, None, decided)
            S["after_reject"] = (M.retract(S["op"], d), state_bound(kappa, d, S["op"]), lam)
            S["trial_state"] = np.array(req.state, np.float32)
            S["damping_after"] = {True: f32clamp(np.float32(req.damping) / np.float32(o.lm_lambda_factor), o.lm_min_lambda, o.lm_max_lambda),
                                  False: None}  # (rejected and yet a LINEARIZE: the level stopped; nothing to compare)
            S["delta_if_rejected"] = (d, 4 * K * EPS * kappa * np.abs(d).max())
        else:
            p, _, pr, _, _, _ = M.dogleg(S["H"], S["b"], req.damping)
            rho = (S["current"] - cost) / pr
            rho_err = (cost_bound(x, ans[0], S["w"]) + S["current_bound"]) / pr + abs(rho) * 4 * K * EPS * cond_inf(S["H"])
            decided = (rho >= o.dogleg_eta1) if abs(rho - o.dogleg_eta1) > rho_err else None
            S["expect"] = ("accept-or-not", None, None, decided)
            S["trial_state"] = np.array(req.state, np.float32)
            r32 = np.float32(req.damping)
            lo, hi = o.dogleg_min_trust_region_radius, o.dogleg_max_trust_region_radius
            grown = None  # undecidable unless both conditions of the growth are clear of rounding
            norm_clear = abs(S["step_norm"] - 0.99 * req.damping) > 4 * K * EPS * cond_inf(S["H"]) * req.damping
            if abs(rho - o.dogleg_eta2) > rho_err and norm_clear:
                grow = rho > o.dogleg_eta2 and S["step_norm"] >= 0.99 * req.damping
                grown = f32clamp(r32 * np.float32(o.dogleg_gamma_increase), lo, hi) if grow else r32
            S["damping_after"] = {True: grown, False: f32clamp(r32 * np.float32(o.dogleg_gamma_decrease), lo, hi)}

    reqs, res = drive(sp, params, factor, api_state(sp, pred32), P, P_prev, True, dev.linearize, dev.trial, watch)
    lib = sp._lib
    # structure that holds whatever the numbers are
    for a, b in zip(reqs, reqs[1:]):
        if a.want == lib.OPT_WANT_TRIAL and b.want != lib.OPT_WANT_TRIAL and method != "GN":
            same = np.array_equal(np.array(b.state, np.float32), np.array(a.state, np.float32))
            # after a trial the loop goes on either at the trial state (accepted) or at the state of the linearisation (rejected / stop)
            assert same or np.array_equal(np.array(b.T, np.float32), np.array(a.T_lin, np.float32)), (method, reg)
        if a.want == lib.OPT_WANT_LINEARIZE and method != "GN":
            assert b.want == lib.OPT_WANT_TRIAL and np.array_equal(np.array(b.T, np.float32), np.array(a.T, np.float32))
    n_lin = sum(r.want == lib.OPT_WANT_LINEARIZE for r in reqs)
    assert res.iterations == n_lin and res.converged == 1 and 1 <= n_lin <= 6
    assert np.array_equal(np.array(res.state, np.float32), np.array(reqs[-1].state, np.float32))
    assert (res.inlier, np.float32(res.error)) == (S["lin"]["inlier"], np.float32(S["lin"]["error"]))  # unweighted, of the last K11
    # the posterior: the inverse of the undamped combined system of the last iteration
    Ppost = np.array(res.posterior_covariance, np.float32).reshape(15, 15).T.astype(f64)
    want = np.linalg.inv(S["H"])
    kappa = cond_inf(S["H"])
    assert np.abs(Ppost - want).max() <= 4 * K_post * EPS * kappa * np.abs(want).max(), (np.abs(Ppost - want).max(), kappa)
    print(f"\n[lio-stepper] {method}-{reg}: {S['steps']} requests, {S['skipped']} undecidable, worst state error / bound "
          f"{S['worst']:.3f}, cond of the last system {kappa:.1f}")
    assert S["skipped"] <= 0.1 * S["steps"]
    # the alignment moved towards the truth
    T_gt = np.asarray(clouds["T_gt"], f64)
    assert np.linalg.norm(np.array(res.state[:3]) - T_gt[:3, 3]) < np.linalg.norm(pred32.p - T_gt[:3, 3])


def serve_constant(lin):
    return (lambda req: lin), (lambda req: (lin["error"], lin["inlier"]))


def requests_of(reqs, want):
    return [r for r in reqs if r.want == want]


@pytest.mark.parametrize("method", ["GN", "LM", "DOGLEG"])
def test_robust_level_schedule(sp, orc, clouds, method):
    """7 iterations over 3 levels: 3 + 2 + 2; scales 8, 4, 2 and 16, 4, 1 (init * factor^l in float32, factor = powf(min / init,
    1 / 2)); lambda / radius restart at every level. Convergence is switched off with criteria of 0."""
    lib = sp._lib
    factor = sp.RegistrationParams(reg_type="GICP", robust_type="HUBER")
    pred32, P, P_prev = start(clouds, scale=1e-3)
    params = lio_params(sp, method, 7, criteria_rotation=0.0, criteria_translation=0.0, auto_scale=True, init_scale=8.0,
                        min_scale=2.0, rotation_init_scale=16.0, rotation_min_scale=1.0, auto_scaling_iter=3)
    dev = OracleDevice(orc, clouds, "GICP", "HUBER")
    reqs, res = drive(sp, params, factor, api_state(sp, pred32), P, P_prev, True, dev.linearize, dev.trial)
    lins = requests_of(reqs, lib.OPT_WANT_LINEARIZE)
    assert sorted({r.level for r in lins}) == [0, 1, 2]
    for r in reqs:  # (the DONE request reports the last level's)
        assert (r.robust_scale, r.rotation_robust_scale) == (np.float32(8.0 * 0.5 ** r.level), np.float32(16.0 * 0.25 ** r.level))
    o = params.optimization
    init = {"GN": o.gn_lambda, "LM": o.lm_init_lambda, "DOGLEG": o.dogleg_initial_trust_region_radius}[method]
    for level in (0, 1, 2):
        first = next(r for r in lins if r.level == level)
        assert first.iteration == 0 and first.damping == np.float32(init)
    budget = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (2, 1)]
    if method != "LM":  # iterations per level: no solve fails here, and a rejected dog-leg step goes on
        assert [(r.level, r.iteration) for r in lins] == budget and res.iterations == 7
        return
    # LM: only an iteration without an accepted trial may end a level before its budget: 1 + max_inner trials, the state unchanged.
    # Every other iteration ends on its accepted trial, after k rejections, and leaves lambda * factor^k / factor behind
    seen = [(r.level, r.iteration) for r in lins]
    assert seen == [b for b in budget if b in seen] and res.iterations == len(seen)
    at = [i for i, r in enumerate(reqs) if r.want == lib.OPT_WANT_LINEARIZE] + [len(reqs) - 1]
    for a, b in zip(at, at[1:]):
        lin, nxt, trials = reqs[a], reqs[b], b - a - 1
        assert all(r.want == lib.OPT_WANT_TRIAL for r in reqs[a + 1:b]) and 2 <= trials <= 1 + o.lm_max_inner_iterations
        if bytes(nxt.state) == bytes(lin.state):  # nothing accepted: the level ends here
            assert trials == 1 + o.lm_max_inner_iterations and (nxt.level, nxt.iteration) != (lin.level, lin.iteration + 1)
        else:
            assert bytes(nxt.state) == bytes(reqs[b - 1].state)
            in_budget = (lin.level, lin.iteration + 1) in budget
            assert ((nxt.level, nxt.iteration) == (lin.level, lin.iteration + 1)) == in_budget  # (criteria 0: no convergence)
            if (nxt.level, nxt.iteration) == (lin.level, lin.iteration + 1) and nxt.want == lib.OPT_WANT_LINEARIZE:
                assert nxt.damping == np.float32(lin.damping * o.lm_lambda_factor ** (trials - 2) / o.lm_lambda_factor)
    assert seen[:5] == budget[:5]  # the first two levels run their whole budget on these clouds


def test_invalid_schedules_fall_back_to_one_level(sp, orc, clouds, capfd):
    lib = sp._lib
    pred32, P, P_prev = start(clouds, scale=1e-3)
    dev = OracleDevice(orc, clouds, "GICP", "HUBER")
    factor = sp.RegistrationParams(reg_type="GICP", robust_type="HUBER", robust_default_scale=3.0,
                                   rotation_constraint_robust_default_scale=7.0)
    bad = [(dict(min_scale=0.0), "[LIORegistration] Invalid geometry robust scale range; disabling auto scaling."),
           (dict(min_scale=10.0), "[LIORegistration] Invalid geometry robust scale range; disabling auto scaling."),
           (dict(rotation_min_scale=10.0), "[LIORegistration] Invalid rotation robust scale range; disabling auto scaling."),
           (dict(auto_scaling_iter=0), "[LIORegistration] auto_scaling_iter must be positive; disabling auto scaling.")]
    for kw, message in bad:
        params = lio_params(sp, "GN", 3, criteria_rotation=0.0, criteria_translation=0.0, auto_scale=True, **kw)
        capfd.readouterr()
        reqs, res = drive(sp, params, factor, api_state(sp, pred32), P, P_prev, True, dev.linearize, dev.trial)
        assert capfd.readouterr().err.strip() == message
        lins = requests_of(reqs, lib.OPT_WANT_LINEARIZE)
        assert len(lins) == 3 and all(r.level == 0 and (r.robust_scale, r.rotation_robust_scale) == (3.0, 7.0) for r in lins)
    # a loss of NONE: no auto scaling and no message
    params = lio_params(sp, "GN", 3, auto_scale=True, min_scale=0.0)
    capfd.readouterr()
    reqs, _ = drive(sp, params, sp.RegistrationParams(), api_state(sp, pred32), P, P_prev, True, dev.linearize, dev.trial)
    assert capfd.readouterr().err == "" and {r.level for r in reqs} == {0} and reqs[0].robust_scale == 10.0


def test_convergence_leaves_the_current_level_only(sp, orc, clouds):
    lib = sp._lib
    pred32, P, P_prev = start(clouds, scale=1e-3)
    dev = OracleDevice(orc, clouds, "GICP", "HUBER")
    factor = sp.RegistrationParams(reg_type="GICP", robust_type="HUBER")
    params = lio_params(sp, "GN", 7, criteria_rotation=1e3, criteria_translation=1e3, auto_scale=True, auto_scaling_iter=3)
    reqs, res = drive(sp, params, factor, api_state(sp, pred32), P, P_prev, True, dev.linearize, dev.trial)
    lins = requests_of(reqs, lib.OPT_WANT_LINEARIZE)
    assert [(r.level, r.iteration) for r in lins] == [(0, 0), (1, 0), (2, 0)] and res.iterations == 3


def test_rejected_dogleg_step_relinearises_at_the_same_state(sp, orc, clouds):
    """eta1 above any gain ratio: every step is rejected; the radius shrinks by gamma_decrease, the iteration counts, the loop goes on."""
    lib = sp._lib
    pred32, P, P_prev = start(clouds, scale=1e-3)
    dev = OracleDevice(orc, clouds, "GICP")
    params = lio_params(sp, "DOGLEG", 4, dogleg_eta1=1e6, dogleg_initial_trust_region_radius=0.5)
    reqs, res = drive(sp, params, sp.RegistrationParams(), api_state(sp, pred32), P, P_prev, True, dev.linearize, dev.trial)
    lins = requests_of(reqs, lib.OPT_WANT_LINEARIZE)
    assert len(lins) == 4 and res.iterations == 4
    for k, r in enumerate(lins):
        assert bytes(r.state) == bytes(lins[0].state) and r.damping == np.float32(0.5 * 0.25 ** k)
    assert np.array_equal(np.array(res.state, np.float32), pred32.pack().astype(np.float32))
    assert [r.want for r in reqs] == [lib.OPT_WANT_LINEARIZE, lib.OPT_WANT_TRIAL, lib.OPT_WANT_TRIAL] * 4 + [lib.OPT_WANT_DONE]


def test_damping_with_forced_decisions(sp, orc, clouds):
    """Trial errors chosen by the test force every decision: LM rejects ten times (lambda doubles, clamped at max_lambda) and the
    level stops with the state unchanged; dog-leg accepts every boundary step with a gain ratio far above eta2 (the radius
    doubles, clamped at its maximum)."""
    lib = sp._lib
    pred32, P, P_prev = start(clouds, scale=1e-3)
    dev = OracleDevice(orc, clouds, "GICP")
    at_lin = lambda req: np.array_equal(np.array(req.T, np.float32), np.array(req.T_lin, np.float32))  # noqa: E731
    params = lio_params(sp, "LM", 3, lm_max_lambda=100.0)
    reqs, res = drive(sp, params, sp.RegistrationParams(), api_state(sp, pred32), P, P_prev, True, dev.linearize,
                      lambda req: dev.trial(req) if at_lin(req) else (1e30, 600))
    trials = requests_of(reqs, lib.OPT_WANT_TRIAL)
    assert [r.want for r in reqs] == [lib.OPT_WANT_LINEARIZE] + [lib.OPT_WANT_TRIAL] * 11 + [lib.OPT_WANT_DONE]
    assert [r.damping for r in trials] == [1.0, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 100.0, 100.0, 100.0]
    assert res.iterations == 1 and np.array_equal(np.array(res.state, np.float32), pred32.pack().astype(np.float32))
    # smaller steps under more damping
    steps = [np.linalg.norm(np.array(r.state, np.float32)[:3] - pred32.p) for r in trials[1:]]
    assert all(a > b for a, b in zip(steps, steps[1:8]))

    params = lio_params(sp, "DOGLEG", 5, criteria_rotation=0.0, criteria_translation=0.0, dogleg_initial_trust_region_radius=0.004,
                        dogleg_max_trust_region_radius=0.02)
    reqs, res = drive(sp, params, sp.RegistrationParams(), api_state(sp, pred32), P, P_prev, True, dev.linearize,
                      lambda req: dev.trial(req) if at_lin(req) else (0.0, 600))
    lins = requests_of(reqs, lib.OPT_WANT_LINEARIZE)
    assert [r.damping for r in lins] == [np.float32(v) for v in (0.004, 0.008, 0.016, 0.02, 0.02)] and res.iterations == 5
    for a, b in zip(lins, lins[1:]):  # each accepted step is as long as its radius
        da = M.St.unpack(np.array(a.state, np.float32))
        db = M.St.unpack(np.array(b.state, np.float32))
        step = np.concatenate([db.p - da.p, M.log_so3(da.R.T @ db.R), db.v - da.v, db.ba - da.ba, db.bg - da.bg])
        assert abs(np.linalg.norm(step) - a.damping) <= 1e-3 * a.damping


@pytest.mark.parametrize("method", ["GN", "LM", "DOGLEG"])
def test_update_bias_false_keeps_the_biases(sp, orc, clouds, method):
    pred32, P, P_prev = start(clouds, scale=1e-3)
    dev = OracleDevice(orc, clouds, "GICP")
    params = lio_params(sp, method, 4)
    reqs, res = drive(sp, params, sp.RegistrationParams(), api_state(sp, pred32), P, P_prev, False, dev.linearize, dev.trial)
    want = pred32.pack().astype(np.float32)[15:]
    for r in reqs:
        assert np.array_equal(np.array(r.state, np.float32)[15:], want)
    assert np.array_equal(np.array(res.state, np.float32)[15:], want)
    assert not np.array_equal(np.array(res.state, np.float32)[:15], pred32.pack().astype(np.float32)[:15])
    # ... and with update_bias the coupled prior moves them
    reqs, res = drive(sp, params, sp.RegistrationParams(), api_state(sp, pred32), P, P_prev, True, dev.linearize, dev.trial)
    assert not np.array_equal(np.array(res.state, np.float32)[15:], want)


def test_edges(sp, orc, clouds, capfd):
    lib = sp._lib
    pred32, P, P_prev = start(clouds, scale=1e-3)
    x0 = pred32.pack().astype(np.float32)
    dev = OracleDevice(orc, clouds, "GICP")
    never = lambda req: pytest.fail("nothing may be asked for")  # noqa: E731
    # total_iterations = 0
    reqs, res = drive(sp, lio_params(sp, "LM", 0), sp.RegistrationParams(), api_state(sp, pred32), P, P_prev, True, never, never)
    assert len(reqs) == 1 and np.array_equal(np.array(res.state, np.float32), x0)
    assert np.array_equal(np.array(res.posterior_covariance, np.float32), cm(P_prev))
    assert (res.iterations, res.inlier, res.converged) == (0, 0, 1) and res.error == np.finfo(np.float32).max
    # an invalid prior (zero covariance): velocity and biases only see the regularisation and a zero gradient
    for method in ("GN", "LM", "DOGLEG"):
        reqs, res = drive(sp, lio_params(sp, method, 3), sp.RegistrationParams(), api_state(sp, pred32), np.zeros((15, 15), np.float32),
                          P_prev, True, dev.linearize, dev.trial)
        got = np.array(res.state, np.float32)
        assert np.array_equal(got[12:], x0[12:]) and not np.array_equal(got[:12], x0[:12]), method
    # a solve that must fail: zero sums, invalid prior, no regularisation, lambda 0 -> the level stops, the state stays.
    # The posterior chain: LDLT(0) is not positive, LDLT(0 + 1e-4 I) is: the second link, (1e-4 I)^-1
    zero = dict(H=np.zeros((6, 6), np.float32), b=np.zeros(6, np.float32), error=0.0, inlier=0)
    params = lio_params(sp, "GN", 3, gn_lambda=0.0, invalid_regularization_factor=0.0)
    capfd.readouterr()
    reqs, res = drive(sp, params, sp.RegistrationParams(), api_state(sp, pred32), np.zeros((15, 15), np.float32), P_prev, True,
                      *serve_constant(zero))
    assert [r.want for r in reqs] == [lib.OPT_WANT_LINEARIZE, lib.OPT_WANT_DONE] and res.iterations == 1
    assert np.array_equal(np.array(res.state, np.float32), x0)
    Ppost = np.array(res.posterior_covariance, np.float32).reshape(15, 15)
    assert np.array_equal(Ppost, np.diag(np.full(15, np.float32(1.0) / np.float32(1e-4), np.float32)))
    assert capfd.readouterr().err == ""
    # the third link: a system that stays indefinite with 1e-4 on its diagonal -> the previous posterior and the warning
    neg = dict(H=(-1e6 * np.eye(6)).astype(np.float32), b=np.ones(6, np.float32), error=1.0, inlier=100)
    for method in ("GN", "LM"):
        params = lio_params(sp, method, 3, gn_lambda=0.0, invalid_regularization_factor=0.0, enable=False)
        capfd.readouterr()
        reqs, res = drive(sp, params, sp.RegistrationParams(), api_state(sp, pred32), np.zeros((15, 15), np.float32), P_prev, True,
                          *serve_constant(neg))
        assert res.iterations == 1 and np.array_equal(np.array(res.state, np.float32), x0), method
        assert np.array_equal(np.array(res.posterior_covariance, np.float32), cm(P_prev))
        assert "[LIORegistration] WARNING: posterior covariance solve failed; keeping previous covariance." in capfd.readouterr().err
    # the first iteration's prior gradient is zero: with zero ICP sums and a valid prior nothing moves, and the posterior is P
    reqs, res = drive(sp, lio_params(sp, "GN", 2, gn_lambda=0.0), sp.RegistrationParams(), api_state(sp, pred32), P, P_prev, True,
                      *serve_constant(zero))
    assert np.array_equal(np.array(res.state, np.float32), x0) and res.iterations == 1  # |delta| = 0 < criteria: converged
    Ppost = np.array(res.posterior_covariance, np.float32).reshape(15, 15).T.astype(np.float64)
    assert np.abs(Ppost - P).max() <= 4 * EPS * cond_inf(P) ** 2 * np.abs(P).max()
    # the same system under the dog-leg: a zero gradient gives a zero step, predicted reduction 0 <= 0: no candidate is tried, the
    # radius shrinks, every iteration counts and the loop goes on at the unchanged state
    # (an identity rotation, so that the residual at the prediction is exactly zero in every iteration)
    upright = sp.IMUState(position=pred32.p.astype(np.float32), velocity=pred32.v.astype(np.float32))
    reqs, res = drive(sp, lio_params(sp, "DOGLEG", 3), sp.RegistrationParams(), upright, P, P_prev, True, *serve_constant(zero))
    assert [r.want for r in reqs] == [lib.OPT_WANT_LINEARIZE, lib.OPT_WANT_TRIAL] * 3 + [lib.OPT_WANT_DONE] and res.iterations == 3
    assert [r.damping for r in requests_of(reqs, lib.OPT_WANT_LINEARIZE)] == [1.0, 0.25, 0.0625]
    assert all(bytes(r.state) == bytes(reqs[0].state) for r in reqs) and np.array_equal(np.array(res.state, np.float32), upright.pack())


def test_icp_weight(sp, orc, clouds):
    """icp_weight = 1 / max(1, 2 error / (dim inlier - 6)) when that dof is > 0 and the error finite and >= 0, else 1."""
    lib = sp._lib
    pred32, P, P_prev = start(clouds, scale=1e-3)
    H = np.eye(6, dtype=np.float32)
    for reg, error, inlier, want in (("GICP", 5000.0, 100, 1.0 / (2 * 5000.0 / 294.0)), ("POINT_TO_PLANE", 5000.0, 100, 94.0 / 1e4),
                                     ("GICP", 10.0, 100, 1.0), ("GICP", 5000.0, 2, 1.0), ("POINT_TO_PLANE", 5000.0, 6, 1.0),
                                     ("GICP", float("inf"), 100, 1.0), ("GICP", -5000.0, 100, 1.0)):
        lin = dict(H=H, b=np.zeros(6, np.float32), error=error, inlier=inlier)
        reqs, _ = drive(sp, lio_params(sp, "LM", 1), sp.RegistrationParams(reg_type=reg), api_state(sp, pred32), P, P_prev, True,
                        lambda req: lin, lambda req: (0.0 if not np.isfinite(error) else error, inlier))
        assert reqs[0].icp_weight == 1.0
        assert abs(reqs[1].icp_weight - want) <= 2 * EPS * want, (reg, error, inlier, reqs[1].icp_weight, want)
