"""pipeline::lidar_odometry::LiDAROdometryPipeline on the device, through the C++ facade at the reference's include paths
(tests/cpp/test_lidar_odometry.cpp) and the example (examples/example_lidar_odometry.cpp), both built here with
tests/cpp/Makefile's flags and libraries (the Makefile is not changed).

What the C++ program holds, on the golden scans (69 k points) or smaller:
  1. the pipeline is the chain: target.ply at t = 0.0 and source.ply at t = 0.1 through process() give first_frame then success, and
     the pose and the preprocessed row counts are those of the same calls made by hand on fresh objects - bit for bit when two hand
     runs agree bit for bit, else within four times their largest entry difference;
  2. that pose lies within 0.05 m and 0.01 per rotation entry of T_target_source.txt;
  3. five frames 0.1 s apart, frame k being target.ply seen from a sensor moved by k * (0.3 m forward, 1 degree yaw), with both
     submap types: every consecutive pair of poses within the same bound of the true relative motion; the voxel hash map declares
     3 keyframes with distance_threshold 0.5 and 1 with inlier_ratio_threshold 1.0; the submap keeps at least min_num_points;
  4. old_timestamp, small_number_of_points and error with their messages, the four timing keys;
  5. the IMU buffer's rules, the initial-alignment gate, GYRO_LIDAR_CV / IMU_SE3 against LIDAR_CV on two identical frames with a
     resting IMU, the velocity-update switch under IMU deskew; the IMU deskew in preprocess and the velocity update on a stamped
     scan at rest (beyond the issue's list: the two paths of process() that nothing else above reaches).

Measured on an MI355X (the program prints every figure before it checks it): two hand runs of the chain are bit-identical and the
pipeline's pose equals them bit for bit (4274 / 4452 preprocessed rows, 983 inliers of 1000); against the ground truth 0.031 m and
0.0048; the drive's relative errors are at most 0.018 m / 0.0031 (occupancy grid) and 0.015 m / 0.0029 (voxel hash map);
|IMU_SE3 - LIDAR_CV| = 3.7e-9, GYRO_LIDAR_CV equals LIDAR_CV; the stamped scan at rest keeps the identity pose (0) through both deskews.
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp")


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
    exe = build(os.path.join(CPP, "test_lidar_odometry.cpp"), os.path.join(CPP, "test_lidar_odometry"))
    r = subprocess.run([exe, GOLD], capture_output=True, text=True, timeout=300)
    print(r.stdout[-12000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
    for name in ("pipeline_is_the_chain", "ground_truth", "drive_occupancy_grid", "drive_voxel_hash_map", "result_codes",
                 "imu_buffer_rules", "initial_alignment_gate", "motion_prediction_modes", "deskew_paths"):
        assert f"[  OK  ] {name}" in r.stdout, name


def test_example(gpu):
    """the example builds and runs the golden pair to the end: first_frame, then success, four stage times per scan"""
    exe = build(os.path.join(ROOT, "examples", "example_lidar_odometry.cpp"), os.path.join(CPP, "example_lidar_odometry"))
    r = subprocess.run([exe, os.path.join(GOLD, "target.ply"), os.path.join(GOLD, "source.ply")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "result 1" in r.stdout and "result 0" in r.stdout and "RESULT " in r.stdout
    for key in ("1. preprocessing", "2. compute covariances", "3. registration", "4. build submap"):
        assert r.stdout.count(key) == 2, key
