"""Host numerics of the odometry loop (csrc/odometry_host.hip) through sycl_points_amd.api against float64 numpy models written
here, and the host-only C++ program of the facade's pipeline classes (tests/cpp/test_lidar_odometry_host.cpp). No GPU.

Bounds (poses with entries <= 10): 1e-5 absolute for rotation entries, roll and pitch, 1e-5 * max(1, |t|) for translations - a few
dozen float32 roundings of 6e-8 each; tests/test_host_terms.py holds the twins of these helpers at 1e-5 / 1e-6. Inputs stay away
from the clamp edges and from equal eigenvalues.
"""
import os
import subprocess

import numpy as np
import pytest

import sycl_points_amd.api as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROT_TOL = 1e-5
G = 9.80665


def trans_tol(t):
    return 1e-5 * max(1.0, float(np.abs(t).max()))


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def log_so3(R):
    R = np.asarray(R, np.float64)
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    th = np.arccos(c)
    if th < 1e-12:
        return np.zeros(3)
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def pose(w, t):
    T = np.eye(4)
    T[:3, :3] = rodrigues(w)
    T[:3, 3] = t
    return T


def assert_pose(T, ref):
    ref = np.asarray(ref, np.float64)
    assert np.abs(ref).max() <= 10.0
    assert np.abs(T[:3, :3] - ref[:3, :3]).max() <= ROT_TOL, np.abs(T[:3, :3] - ref[:3, :3]).max()
    assert np.abs(T[:3, 3] - ref[:3, 3]).max() <= trans_tol(ref[:3, 3]), np.abs(T[:3, 3] - ref[:3, 3]).max()
    assert np.array_equal(T[3], [0, 0, 0, 1])


# ------------------------------------------------------------------------------------------------ motion prediction
class Model:
    """AdaptiveMotionPredictor / MotionPredictor (adaptive_motion_predictor.hpp:54-133, motion_predictor.hpp:60-76) in float64"""

    def __init__(self, params):
        self.p = params
        self.lin = None
        self.ang = None

    @staticmethod
    def factor(axis, H_block, inlier):
        ratio = np.linalg.eigvalsh(H_block.astype(np.float64)).min() / inlier
        score = np.clip((ratio - axis.min_eigenvalue_low) / max(axis.min_eigenvalue_high - axis.min_eigenvalue_low, 1e-6), 0.0, 1.0)
        return axis.factor_max * (1 - score) + axis.factor_min * score

    def predict(self, v, w, odom, dt, H=None, inlier=0, registrated=False, gyro=None, se3=None):
        if self.p.mode == "IMU_SE3" and se3 is not None:
            return np.asarray(se3, np.float64), None
        fr, ft = self.p.rotation.factor_max, self.p.translation.factor_max
        if registrated and inlier > 0:
            fr = self.factor(self.p.rotation, H[:3, :3], inlier)
            ft = self.factor(self.p.translation, H[3:, 3:], inlier)
        a = self.p.velocity_ema_alpha
        v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
        self.lin = v if self.lin is None else a * v + (1 - a) * self.lin
        self.ang = w if self.ang is None else a * w + (1 - a) * self.ang
        odom = np.asarray(odom, np.float64)
        n = np.linalg.norm(self.ang)
        T = np.eye(4)
        T[:3, 3] = odom[:3, 3] + odom[:3, :3] @ (self.lin * dt * ft)
        T[:3, :3] = odom[:3, :3] @ (rodrigues(self.ang / n * (n * dt * fr)) if n > 1e-6 else np.eye(3))
        if self.p.mode == "GYRO_LIDAR_CV" and gyro is not None:
            rel = np.linalg.inv(odom) @ T
            rel[:3, :3] = gyro
            T = odom @ rel
        return T, (fr, ft)


def hessian(rot_ratios, trans_ratios, inlier, seed):
    """H_raw (6x6) whose rotation / translation blocks have the given eigenvalues per inlier, in random bases, plus coupling blocks
    the predictor must not read"""
    rs = np.random.RandomState(seed)
    H = rs.uniform(-1, 1, (6, 6))
    H = H + H.T
    for o, ratios in ((0, rot_ratios), (3, trans_ratios)):
        Q = rodrigues(rs.uniform(-1, 1, 3))
        H[o:o + 3, o:o + 3] = Q @ np.diag(np.asarray(ratios, np.float64) * inlier) @ Q.T
    return H.astype(np.float32)


ODOM = pose([0.2, -0.1, 0.4], [2.0, -1.0, 0.5])
ROT_CASES = {"below": 2.0, "between": 7.5, "above": 15.0}  # rotation bounds 5 / 10
TRANS_CASES = {"below": 0.5, "between": 4.0, "above": 20.0}  # translation bounds 1 / 10


@pytest.mark.parametrize("rot", list(ROT_CASES))
@pytest.mark.parametrize("trans", list(TRANS_CASES))
def test_degeneracy_factors_are_the_interpolation(rot, trans):
    """the smallest eigenvalue per inlier below `low`, between the bounds and above `high`, for both blocks independently"""
    params = sp.MotionPredictionParams(mode="LIDAR_CV")
    inlier = 800
    H = hessian([ROT_CASES[rot], 40.0, 90.0], [TRANS_CASES[trans], 35.0, 70.0], inlier, seed=5)
    got = sp.MotionPredictor(params)
    T = got.predict([1.0, 2.0, 3.0], [0.3, -0.2, 0.1], ODOM, 0.1, H_raw=H, inlier=inlier, registrated=True)
    ref, (fr, ft) = Model(params).predict([1.0, 2.0, 3.0], [0.3, -0.2, 0.1], ODOM, 0.1, H=H, inlier=inlier, registrated=True)
    want = {"below": 1.0, "above": 0.2}
    want_r = want.get(rot, 1.0 - 0.8 * (7.5 - 5.0) / 5.0)
    want_t = want.get(trans, 1.0 - 0.8 * (4.0 - 1.0) / 9.0)
    print(f"rotation {rot}: {got.last_factors[0]:.7f} (interpolation {want_r:.7f}); translation {trans}: {got.last_factors[1]:.7f} ({want_t:.7f})")
    assert abs(fr - want_r) < 1e-6 and abs(ft - want_t) < 1e-6  # (the model agrees with the closed form)
    assert abs(got.last_factors[0] - want_r) <= 1e-5 and abs(got.last_factors[1] - want_t) <= 1e-5
    if rot != "between":
        assert got.last_factors[0] == np.float32(want_r)  # clamped: exactly factor_max / factor_min
    if trans != "between":
        assert got.last_factors[1] == np.float32(want_t)
    assert_pose(T, ref)


@pytest.mark.parametrize("registrated,inlier", [(False, 800), (True, 0)])
def test_no_registration_gives_factor_max(registrated, inlier):
    params = sp.MotionPredictionParams(rotation=sp.AdaptiveAxisParams(0.2, 0.9, 5.0, 10.0), translation=sp.AdaptiveAxisParams(0.3, 0.8, 1.0, 10.0),
                                       mode="LIDAR_CV")
    H = hessian([15.0, 40.0, 90.0], [20.0, 35.0, 70.0], 800, seed=6)  # would give factor_min
    got = sp.MotionPredictor(params)
    T = got.predict([1.0, 2.0, 3.0], [0.3, -0.2, 0.1], ODOM, 0.1, H_raw=H, inlier=inlier, registrated=registrated)
    assert got.last_factors == (float(np.float32(0.9)), float(np.float32(0.8)))
    ref, _ = Model(params).predict([1.0, 2.0, 3.0], [0.3, -0.2, 0.1], ODOM, 0.1, H=H, inlier=inlier, registrated=registrated)
    assert_pose(T, ref)
    no_H = sp.MotionPredictor(params).predict([1.0, 2.0, 3.0], [0.3, -0.2, 0.1], ODOM, 0.1)  # H_raw is not needed then
    assert np.array_equal(no_H, T)


def test_velocity_average_over_three_calls():
    params = sp.MotionPredictionParams(velocity_ema_alpha=0.5, mode="LIDAR_CV")
    got, ref = sp.MotionPredictor(params), Model(params)
    calls = [([1.0, 2.0, 3.0], [0.3, -0.2, 0.1]), ([3.0, -2.0, 1.0], [-0.1, 0.4, 0.2]), ([-1.0, 0.5, 2.0], [0.2, 0.2, -0.6])]
    for v, w in calls:
        T = got.predict(v, w, ODOM, 0.5)
        Tr, _ = ref.predict(v, w, ODOM, 0.5)
        assert_pose(T, Tr)
        assert np.abs(np.array(got.state.linear) - ref.lin).max() <= 1e-6 and np.abs(np.array(got.state.angular) - ref.ang).max() <= 1e-6
    # s3 = v3 / 2 + v2 / 4 + v1 / 4
    assert np.allclose(ref.lin, 0.5 * np.array(calls[2][0]) + 0.25 * np.array(calls[1][0]) + 0.25 * np.array(calls[0][0]), atol=1e-12)
    # alpha = 1 (the default) keeps nothing of the past
    raw = sp.MotionPredictor(sp.MotionPredictionParams(mode="LIDAR_CV"))
    for v, w in calls:
        T = raw.predict(v, w, ODOM, 0.5)
    assert_pose(T, Model(sp.MotionPredictionParams(mode="LIDAR_CV")).predict(*calls[2], ODOM, 0.5)[0])


def test_identity_branch_below_1e_6_rad_per_second():
    """1e-7 rad/s is no rotation however long the interval (over 1e4 s it would have been 1e-3 rad); 1e-3 rad/s is one"""
    params = sp.MotionPredictionParams(mode="LIDAR_CV")
    slow = sp.MotionPredictor(params).predict([0.0, 0.0, 0.0], [0.0, 0.0, 1e-7], ODOM, 1e4)
    assert_pose(slow, ODOM)
    assert np.abs(slow[:3, :3] - ODOM[:3, :3] @ rodrigues([0, 0, 1e-3])).max() > 5e-4
    turn = sp.MotionPredictor(params).predict([0.0, 0.0, 0.0], [0.0, 0.0, 1e-3], ODOM, 100.0)
    assert_pose(turn, Model(params).predict([0.0, 0.0, 0.0], [0.0, 0.0, 1e-3], ODOM, 100.0)[0])
    assert np.abs(turn[:3, :3] - ODOM[:3, :3]).max() > 0.05


def test_gyro_fusion_keeps_the_constant_velocity_translation():
    """the reference's own known answer (cpp/tests/test_lidar_odometry_imu.cpp:108-127)"""
    params = sp.MotionPredictionParams()  # GYRO_LIDAR_CV
    odom = pose([0, 0, 0], [2.0, -1.0, 0.5])
    dR = rodrigues([0, 0, 0.4])
    fused = sp.MotionPredictor(params).predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], odom, 1.0, gyro_delta_rotation_lidar=dR)
    assert np.abs(fused[:3, 3] - (odom[:3, 3] + [1.0, 2.0, 3.0])).max() <= trans_tol(fused[:3, 3])
    assert np.abs(fused[:3, :3] - dR).max() <= ROT_TOL
    # from a rotated pose: the model's composition odom * (odom^-1 * prediction with the gyro rotation)
    got = sp.MotionPredictor(params).predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0, gyro_delta_rotation_lidar=dR)
    assert_pose(got, Model(params).predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0, gyro=dR)[0])
    # without the candidate, and in LIDAR_CV with it, the constant-velocity rotation stays
    cv = Model(sp.MotionPredictionParams(mode="LIDAR_CV")).predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0)[0]
    assert_pose(sp.MotionPredictor(params).predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0), cv)
    assert_pose(sp.MotionPredictor(sp.MotionPredictionParams(mode="LIDAR_CV")).predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0,
                                                                                       gyro_delta_rotation_lidar=dR), cv)


def test_imu_se3_returns_the_candidate_unchanged():
    params = sp.MotionPredictionParams(mode="IMU_SE3")
    cand = pose([0.3, 0.1, -0.2], [4.0, 5.0, -6.0]).astype(np.float32)
    mp = sp.MotionPredictor(params)
    T = mp.predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0, imu_se3_pose=cand, gyro_delta_rotation_lidar=rodrigues([0, 0, 0.4]))
    assert np.array_equal(T, cand)
    assert mp.state.has_linear == 0 and mp.state.has_angular == 0  # the averages are not touched on that path
    # without the candidate IMU_SE3 predicts with constant velocity
    assert_pose(mp.predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0), Model(params).predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0)[0])
    # another mode ignores the candidate
    other = sp.MotionPredictor(sp.MotionPredictionParams(mode="LIDAR_CV")).predict([1.0, 2.0, 3.0], [0.2, 0.0, 0.0], ODOM, 1.0, imu_se3_pose=cand)
    assert not np.array_equal(other, cand)


def test_velocity_from_a_pose_pair():
    prev, cur = ODOM, ODOM @ pose([0.02, -0.05, 0.08], [0.3, -0.1, 0.05])
    lin, speed, axis = sp.velocity_from_poses(prev, cur, 0.1)
    delta = np.linalg.inv(prev) @ cur
    assert np.abs(lin - delta[:3, 3] / 0.1).max() <= trans_tol(delta[:3, 3] / 0.1)
    w = log_so3(delta[:3, :3]) / 0.1
    assert speed > 0 and abs(np.linalg.norm(axis) - 1) <= 1e-6
    assert np.abs(speed * axis - w).max() <= 1e-5 * max(1.0, np.abs(w).max())
    lin, speed, axis = sp.velocity_from_poses(ODOM.astype(np.float32), ODOM.astype(np.float32), 0.1)
    assert speed <= 1e-5 and np.abs(lin).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ keyframe decision
BIG = dict(distance_threshold=1e6, angle_threshold_degrees=1e6, time_threshold_seconds=1e6)


def test_keyframe_distance_threshold():
    last = np.eye(4)
    for x, want in ((1.999, False), (2.0, True), (2.001, True)):  # |(2, 0, 0)| is exactly the threshold: counts
        kf, dist, ang, dt = sp.keyframe_decision(last, pose([0, 0, 0], [x, 0, 0]), 1.0, 1.5, **dict(BIG, distance_threshold=2.0))
        assert kf is want and abs(dist - x) <= 1e-6 and ang == 0.0 and dt == 0.5
    # from a rotated keyframe the distance is that of the relative pose
    cur = ODOM @ pose([0, 0, 0], [1.2, -1.6, 0.0])
    assert sp.keyframe_decision(ODOM, cur, 1.0, 1.5, **dict(BIG, distance_threshold=1.99))[0]
    assert not sp.keyframe_decision(ODOM, cur, 1.0, 1.5, **dict(BIG, distance_threshold=2.01))[0]


def test_keyframe_angle_threshold():
    last = ODOM
    cur = ODOM @ pose(np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74]) * np.radians(20.0), [0, 0, 0])
    _, dist, ang, _ = sp.keyframe_decision(last, cur, 1.0, 1.5, **BIG)
    assert abs(ang - 20.0) <= 1e-3 and dist <= 1e-6  # degrees, of the relative rotation
    for thr, want in ((ang + 0.01, False), (ang, True), (ang - 0.01, True)):  # exactly at the threshold counts
        assert sp.keyframe_decision(last, cur, 1.0, 1.5, **dict(BIG, angle_threshold_degrees=thr))[0] is want


def test_keyframe_time_threshold():
    T = np.eye(4)
    for now, want in ((1.999, False), (2.0, True), (2.001, True)):
        kf, _, _, dt = sp.keyframe_decision(T, T, 1.0, now, **dict(BIG, time_threshold_seconds=1.0))
        assert kf is want and abs(dt - (now - 1.0)) <= 1e-12
    for last_time in (-1.0, 0.0):  # not > 0.0: no keyframe time yet, the difference is infinite
        kf, _, _, dt = sp.keyframe_decision(T, T, last_time, 0.5, **BIG)
        assert kf and dt == np.finfo(np.float64).max
    assert not sp.keyframe_decision(T, T, 1e-9, 0.5, **BIG)[0]


# ------------------------------------------------------------------------------------------------ initial alignment
def from_two_vectors(a, b):
    """the minimum rotation taking a onto b (Quaternionf::FromTwoVectors), float64"""
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    axis = np.cross(a, b)
    s, c = np.linalg.norm(axis), a @ b
    return rodrigues(axis / s * np.arctan2(s, c)) if s > 0 else np.eye(3)


def tilted_force(roll, pitch):
    """what an accelerometer at rest reads with R_world_body = Ry(pitch) Rx(roll)"""
    R = rodrigues([0, pitch, 0]) @ rodrigues([roll, 0, 0])
    return R.T @ np.array([0.0, 0.0, G])


def stationary_buffer(n=121, rate=100.0, t0=50.0, seed=1):
    rs = np.random.RandomState(seed)
    stamps = t0 + np.arange(n) / rate
    gyro = np.array([0.004, -0.002, 0.003]) + rs.normal(0, 1e-3, (n, 3))
    accel = tilted_force(np.radians(10.0), np.radians(-5.0)) + rs.normal(0, 2e-2, (n, 3))
    return stamps, gyro.astype(np.float32), accel.astype(np.float32)


def test_alignment_recovers_roll_pitch_and_gyro_bias():
    stamps, gyro, accel = stationary_buffer()
    r = sp.estimate_initial_alignment(stamps, gyro, accel)
    assert r.success and r.error_message == ""
    win = stamps >= stamps[-1] - 1.0
    win[np.flatnonzero(win)[0] - 1] = stamps[np.flatnonzero(win)[0]] > stamps[-1] - 1.0 + 1e-6
    a_mean, g_mean = accel[win].astype(np.float64).mean(0), gyro[win].astype(np.float64).mean(0)
    R = from_two_vectors(a_mean, np.array([0.0, 0.0, 1.0]))
    roll, pitch = np.arctan2(R[2, 1], R[2, 2]), np.arcsin(-R[2, 0])
    print(f"roll {r.roll_rad:.7f} (model {roll:.7f}), pitch {r.pitch_rad:.7f} (model {pitch:.7f}), window {r.window_size}")
    assert r.window_size == int(win.sum())
    assert abs(r.roll_rad - roll) <= 1e-5 and abs(r.pitch_rad - pitch) <= 1e-5
    assert abs(roll - np.radians(10.0)) < 2e-3 and abs(pitch - np.radians(-5.0)) < 2e-3  # (the noise moves the mean a little)
    assert np.abs(r.R_world_imu - R).max() <= ROT_TOL
    yaw = sp.yaw_from_rotation(r.R_world_imu)
    assert abs(yaw - np.arctan2(R[1, 0], R[0, 0])) <= 1e-5 and abs(yaw) < 0.02  # the minimum rotation's yaw: about roll * pitch / 2
    assert np.array_equal(r.gyro_bias, g_mean.astype(np.float32))  # the mean, accumulated in double
    assert np.array_equal(r.accel_mean, a_mean.astype(np.float32))
    assert np.abs(r.gyro_std - gyro[win].astype(np.float64).std(0)).max() <= 1e-7
    assert np.abs(r.accel_std - accel[win].astype(np.float64).std(0)).max() <= 1e-6
    assert abs(r.accel_norm - np.linalg.norm(a_mean)) <= 1e-5
    # without noise the tilt comes back itself; the configured bias is kept when it is not to be estimated
    n = 121
    exact = sp.estimate_initial_alignment(stamps, np.zeros((n, 3)), np.tile(tilted_force(np.radians(10.0), np.radians(-5.0)), (n, 1)),
                                          params=sp.InitialAlignmentParams(estimate_gyro_bias=False), current_bias=[0.1, 0.2, 0.3, 0, 0, 0])
    assert abs(exact.roll_rad - np.radians(10.0)) <= 1e-5 and abs(exact.pitch_rad - np.radians(-5.0)) <= 1e-5
    assert np.array_equal(exact.gyro_bias, np.array([0.1, 0.2, 0.3], np.float32))
    # a gravity vector that is not along z: the measured force is taken onto -gravity
    g_w = np.array([0.0, -G, 0.0])
    other = sp.estimate_initial_alignment(stamps, gyro, accel, gravity_world=g_w)
    assert np.abs(other.R_world_imu - from_two_vectors(a_mean, -g_w)).max() <= ROT_TOL


def test_alignment_early_returns_and_their_messages():
    stamps, gyro, accel = stationary_buffer()
    P = sp.InitialAlignmentParams

    def msg(*a, **k):
        r = sp.estimate_initial_alignment(*a, **k)
        assert not r.success
        return r.error_message

    assert msg(stamps, gyro, accel, gravity_world=(0.0, 0.0, 1e-4)) == "gravity vector is (near) zero"
    assert msg(stamps[:1], gyro[:1], accel[:1]) == "IMU buffer has fewer than 2 samples"
    assert msg([], np.zeros((0, 3)), np.zeros((0, 3))) == "IMU buffer has fewer than 2 samples"
    assert msg(stamps[:100], gyro[:100], accel[:100]) == "IMU buffer spans less than required_duration_sec"  # 0.99 s
    assert sp.estimate_initial_alignment(stamps[:101], gyro[:101], accel[:101]).success  # 1.00 s: the span itself suffices
    assert msg(stamps, gyro, accel, params=P(required_duration_sec=-1.0)) == "no IMU samples in required window"
    shaky = gyro.copy()
    shaky[::2, 1] += 0.05
    assert msg(stamps, shaky, accel) == "gyro_std exceeds threshold (robot not stationary?)"
    bumpy = accel.copy()
    bumpy[::2, 0] += 1.0
    assert msg(stamps, gyro, bumpy) == "accel_std exceeds threshold (robot not stationary?)"
    assert msg(stamps, shaky, bumpy) == "gyro_std exceeds threshold (robot not stationary?)"  # the gyro test comes first
    assert msg(stamps, gyro, accel * np.float32(1.1)) == "|a_mean| - |gravity| exceeds threshold (unmodelled accel bias?)"
    a_mean = accel[20:].astype(np.float64).mean(0)
    assert msg(stamps, gyro, accel, current_bias=[0, 0, 0, *a_mean]) == "bias-corrected accel magnitude is (near) zero"
    # the statistics are reported with a stationarity failure too
    r = sp.estimate_initial_alignment(stamps, shaky, accel)
    assert r.gyro_std[1] > 0.02 and abs(r.accel_norm - G) < 0.1 and r.window_size == 101


def test_alignment_window_takes_one_earlier_sample():
    """samples every 0.5 s from 0.45: the window [1.0, 2.0] starts with the sample at 1.45, so the one at 0.95 joins it; with a
    sample exactly at 1.0 nothing is added"""
    force = tilted_force(0.1, 0.05)
    stamps = np.array([0.0, 0.45, 0.95, 1.45, 1.95, 2.0])
    gyro = np.array([[9.0, 9, 9], [8.0, 8, 8], [0.4, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [0.3, 0, 0]], np.float32)
    accel = np.tile(force, (6, 1)).astype(np.float32)
    r = sp.estimate_initial_alignment(stamps, gyro, accel, bypass_stationarity=True)
    assert r.success and r.window_size == 4
    assert np.array_equal(r.gyro_bias, np.array([0.25, 0, 0], np.float64).astype(np.float32))
    stamps[2] = 1.0
    r = sp.estimate_initial_alignment(stamps, gyro, accel, bypass_stationarity=True)
    assert r.success and r.window_size == 4 and abs(r.gyro_bias[0] - 0.25) <= 1e-7  # 1.0 itself is in the window
    stamps[2] = 1.0 - 1e-4  # outside, but the window would start 0.45 s late without it
    assert sp.estimate_initial_alignment(stamps, gyro, accel, bypass_stationarity=True).window_size == 4
    stamps = np.array([0.0, 0.45, 0.95, 1.0 + 5e-7, 1.95, 2.0])  # the first window sample within 1e-6 of the start: no extension
    assert sp.estimate_initial_alignment(stamps, gyro, accel, bypass_stationarity=True).window_size == 3


def test_unstationary_buffer_passes_only_with_bypass():
    stamps, gyro, accel = stationary_buffer()
    shaky = gyro.copy()
    shaky[::2, 1] += 0.05
    assert not sp.estimate_initial_alignment(stamps, shaky, accel).success
    r = sp.estimate_initial_alignment(stamps, shaky, accel, bypass_stationarity=True)
    assert r.success and r.error_message == ""
    assert abs(r.roll_rad - np.radians(10.0)) < 2e-3 and abs(r.gyro_bias[1] - (-0.002 + 0.025)) < 1e-3  # the polluted mean


def test_yaw_from_rotation():
    for yaw in (-2.5, -0.3, 0.0, 1.2, 3.0):
        R = rodrigues([0, 0, yaw]) @ rodrigues([0, 0.3, 0]) @ rodrigues([-0.2, 0, 0])
        assert abs(sp.yaw_from_rotation(R) - yaw) <= 1e-6
    assert sp.yaw_from_rotation(rodrigues([0, np.pi / 2, 0]).round(12)) == 0.0  # the first column points along z


# ------------------------------------------------------------------------------------------------ the facade's host classes
def test_host_cpp_program(tmp_path):
    """tests/cpp/test_lidar_odometry_host.cpp with tests/cpp/Makefile's flags (the Makefile is not changed): try_align waiting,
    succeeding and forcing after max_wait_sec; IMUVelocityCorrector's two formulas on a hand-computed case and its fallback; the
    parameter defaults and string conversions; what make_registration_pipeline_params() copies; MotionPredictor through the
    reference's types. No device is touched."""
    from sycl_points_amd import _lib

    _lib.build()
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "test_lidar_odometry_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_lidar_odometry_host.cpp"), "-o", exe,
                           f"-L{libdir}", "-lsycl_points_amd", f"-Wl,-rpath,{libdir}", f"-L{rocm}/lib", "-lamdhip64",
                           f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-6000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
