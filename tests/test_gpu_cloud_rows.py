"""The C++ facade on clouds that carry some of the optional attributes and lack the others (tests/cpp/test_cloud_rows.cpp): all 32
subsets of covs / normals / rgb / intensities / timestamp_offsets at N = 1, 64, 65, 257 and 1030, every row tagged with its index,
through everything that treats the attributes alike: box_filter, random_sampling, angle_incidence_filter, OutlierRemoval::radius,
erase, extend, the copy constructor, VoxelGrid and PolarGrid. Rows are moved, not computed: every comparison is exact."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def test_cpp_facade(sp):
    """tests/cpp/test_cloud_rows.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_cloud_rows")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include",
                           "-D__HIP_PLATFORM_AMD__", "-Wall", "-Wno-unused-value", "-Wno-unused-result",
                           os.path.join(cpp, "test_cloud_rows.cpp"), "-o", exe, f"-L{lib}", "-lsycl_points_amd", f"-Wl,-rpath,{lib}",
                           f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
