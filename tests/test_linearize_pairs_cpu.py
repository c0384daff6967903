"""The per-point algebra of the prepared GICP / point-to-distribution linearisation on the host (csrc/sp_linearize.h,
linearize_terms: the function the kernels' fused_math calls) against a plain scalar restatement of its formulas, bit for bit:
tests/cpp/test_linearize_pairs.cpp, a program with its own main, built with hipcc's host compiler only (the header is HIP source)
and -ffp-contract=off as the library is. 100 000 random correspondences through GICP and point-to-distribution, the five losses,
the 28 terms and the error-only form; a rotation with nine distinct non-zero entries, |det| < 1e-6, a zero source covariance,
negative coordinates. Once more, a fifth of the cases, as a stand-alone binary under -fsanitize=address,undefined.

Also: the two translation units that run the algebra are built without SLP vectorisation (csrc/Makefile), which is where this
change's time comes from — the flag must not get lost."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_linearize_pairs.cpp")


def hipcc():
    exe = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(exe):
        pytest.fail("hipcc not found: the library itself cannot be built without it")
    return exe


def build(out, *extra):
    subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", "-ffp-contract=off", "-Wall", *extra, SRC,
                           "-o", out])
    return out


def run(exe, *args):
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    return r


def test_terms_bit_equal_to_scalar_restatement(tmp_path):
    r = run(build(str(tmp_path / "test_linearize_pairs"), "-O2"))
    assert r.returncode == 0, r.stdout
    m = re.search(r"(\d+) cases: (\d+) values compared, (\d+) differ; Zero inverse (\d+), zero source covariance (\d+), "
                  r"negative coordinates (\d+), rotations with nine distinct non-zero entries (\d+)", r.stdout)
    assert m, r.stdout
    cases, compared, differ, zero_inv, zero_cs, negative, distinct = map(int, m.groups())
    assert cases == 100000 and compared == cases * 2 * 5 * 29 and differ == 0
    assert zero_inv > 1000 and zero_cs > 1000 and negative > 1000 and distinct >= cases // 4


def test_under_address_and_undefined_sanitizers(tmp_path):
    exe = build(str(tmp_path / "test_linearize_pairs_san"), "-O1", "-g", "-fsanitize=address,undefined",
                "-fno-sanitize-recover=undefined")
    r = run(exe, "20000")
    assert r.returncode == 0, r.stdout
    assert "0 differ" in r.stdout and "ERROR" not in r.stdout and "runtime error" not in r.stdout


def test_units_of_the_linearisation_are_built_without_slp():
    with open(os.path.join(ROOT, "sycl_points_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^build/registration\.o build/registration_opt\.o: HIPFLAGS \+= -fno-slp-vectorize$", mk, re.M)
