"""pipeline::lidar_inertial_odometry::LidarInertialOdometryPipeline on the device, through the C++ facade at the reference's include
paths (tests/cpp/test_lidar_inertial_odometry.cpp) and the example (examples/example_lidar_inertial_odometry.cpp), both built here
with tests/cpp/Makefile's flags and libraries (the Makefile is not changed).

What the C++ program holds, on the golden scans (69 k points) or smaller, with T_imu_to_lidar = identity, an IMU at 200 Hz, a first
stamp of 1.0 and the noise densities of the reference's config/lidar_inertial_odometry.yaml:
  1. pipeline_is_the_chain: target.ply at 1.0 and source.ply at 1.1 with a resting IMU give first_frame then success, and pose, state
     (21 floats), posterior covariance and preprocessed row counts are those of the same calls made by hand on fresh objects
     (PCProcessor, Submap, an IMUPreintegration reset and read through sp_lio_reset_covariance_host / sp_lio_predict_state_host,
     LIORegistration::align, sp_lio_clamp_bias_host) - bit for bit when two hand runs agree bit for bit, else within four times
     their largest entry difference;
  2. drive_from_rest, both submap types: five frames 0.1 s apart from rest at 4 m/s^2 and 10 deg/s, the IMU reading R^T (a - g) and
     (0, 0, w): every consecutive pair of poses within 0.05 m / 0.01 per rotation entry of the true relative motion, the final
     velocity within 0.5 m/s of the true 1.6 m/s;
  3. imu_only: a 50-point frame 3 returns imu_only with its message, a zeroed registration result, and state, pose and covariance equal
     a hand-integrated window from the state read before the call, bit for bit; frame 4 registers again and lies within the drive's
     bound of the truth (from frame 2, the last registered one); a 50-point FIRST frame returns small_number_of_points and the next
     full frame equals case 1's first frame bit for bit;
  4. result_codes: old_timestamp, error with "preprocess: ..." (the IMU deskew refuses a scan without a queue), the four timing keys
     with "3. lio registration";
  5. bias_rules: freeze_on_low_excitation at rest leaves both biases bit-identical to the parameters, the pose at the identity
     within 1e-4 and |v| <= 1e-3; max_gyro_bias 0.01 clamps a gyro bias of 0.02;
  6. invalid_prior: all noise densities 0 (the alignment's regularisation branch): success, finite state and covariance, identity
     within 1e-4;
  7. initial_alignment: the gate, the first frame's rotation Rz(30 deg) R_gravity_lidar bit for bit with the estimator called by
     hand, the estimator's gyro bias, imu.enable forced and the buffer widened to 1.2 s;
  8. deskew_uses_state: the caller's stamped scan equals a hand deskew with the state's bias and velocity, bit for bit, twice.
The program prints every figure before it checks it; the measured ones are in DESIGN.md 4.16.
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp")
CASES = ("pipeline_is_the_chain", "drive_from_rest", "imu_only", "result_codes", "bias_rules", "invalid_prior", "initial_alignment",
         "deskew_uses_state")


def build(source, exe):
    """g++ with tests/cpp/Makefile's CXXFLAGS and LIBS"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", source, "-o", exe, f"-L{libdir}", "-lsycl_points_amd",
                           f"-Wl,-rpath,{libdir}", f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib"])
    return exe


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from sycl_points_amd import _lib

    _lib.build()


def test_cpp_pipeline(gpu):
    exe = build(os.path.join(CPP, "test_lidar_inertial_odometry.cpp"), os.path.join(CPP, "test_lidar_inertial_odometry"))
    r = subprocess.run([exe, GOLD], capture_output=True, text=True, timeout=300)
    print(r.stdout[-20000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-8000:]
    assert " 0 failed" in r.stdout
    for name in CASES:
        assert f"[  OK  ] {name}" in r.stdout, name


def test_example(gpu):
    """the example builds and runs the golden pair to the end: first_frame, then success, four stage times per scan, the final state"""
    exe = build(os.path.join(ROOT, "examples", "example_lidar_inertial_odometry.cpp"), os.path.join(CPP, "example_lidar_inertial_odometry"))
    r = subprocess.run([exe, os.path.join(GOLD, "target.ply"), os.path.join(GOLD, "source.ply")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "result 1" in r.stdout and "result 0" in r.stdout and "RESULT " in r.stdout and "STATE velocity" in r.stdout
    for key in ("1. preprocessing", "2. compute covariances", "3. lio registration", "4. build submap"):
        assert r.stdout.count(key) == 2, key
