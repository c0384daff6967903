"""The wave form of the iteration finish (csrc/sp_wave_solve.h: the pivoted 6x6 LDL^T solve and the Gauss-Newton pose update on the
lanes of one wave) in its host lockstep form — the same schedule, sixteen lane states stepped side by side — against the one-lane
code it replaces, bit for bit: tests/cpp/test_wave_solve.cpp, a program with its own main, built with hipcc's host compiler only (the
header is HIP source) and -ffp-contract=off as the library is.

Solver (x, dmin and the ok flag against ldlt6_solve): all 720 orderings of a strongly diagonal matrix's diagonal magnitudes (every
exchange target at every step); equal |diagonal| pairs and triples in every position with every sign pattern, all-equal diagonals
of mixed sign (the lowest index must win a tie); zero pivots over a zero column (ok, guarded y = 0) and over a non-zero column at
every step (not ok, x = 0); a D entry at FLT_MIN and one ulp either side, either sign, in every position; entries scaled by 1e-30
and 1e30; NaN and +-inf in every entry of H and of rhs; 2000 random SPD systems J^T J + I as tests/test_cabi.py makes them.
Update (T and delta8 against sp_gn_update_host): every system above, and steps from 1e-9 to 4 rad (below and above the
theta < 1e-6 branch, theta of order 1 and past pi), criteria 0 and 1e-3, criteria at |delta| and one ulp either side of it.

The inputs discriminate: the same wave form with ONE change of order — the back substitution subtracting in descending j —
differs from ldlt6_solve on 1689 of the 2000 random systems (84 %, measured on the CPU); the test asks for at least half."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_wave_solve.cpp")
LIBDIR = os.path.join(ROOT, "sycl_points_amd", "lib")


def hipcc():
    exe = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(exe):
        pytest.fail("hipcc not found: the library itself cannot be built without it")
    return exe


def build_program(out, *extra):
    """The program links the library for the one-lane host twins (sp_gn_update_host, sp_se3_exp_host)."""
    from sycl_points_amd import _lib

    _lib.build()  # nothing happens when the library is current
    subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", "-ffp-contract=off", "-Wall", *extra, SRC,
                           "-o", out, f"-L{LIBDIR}", "-lsycl_points_amd", f"-Wl,-rpath,{LIBDIR}"])
    return out


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = build_program(str(tmp_path_factory.mktemp("wave_solve") / "test_wave_solve"), "-O2")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    return r.stdout


GROUPS = {"orderings": 720, "ties and signs": 204, "zero pivot, zero column": 7, "zero pivot, non-zero column": 15,
          "FLT_MIN guard": 36, "scaled 1e-30 / 1e30": 100, "NaN and inf": 81, "random SPD": 2000}


def test_solve_bit_equal_to_one_lane_solver(output):
    for name, count in GROUPS.items():
        m = re.search(rf"solve, {re.escape(name)}: (\d+) systems, (\d+) differ, (\d+) not ok", output)
        assert m, (name, output)
        n, differ, not_ok = map(int, m.groups())
        assert n == count and differ == 0, (name, output)
        if name == "zero pivot, non-zero column":
            assert not_ok == n
        if name in ("orderings", "ties and signs", "zero pivot, zero column", "FLT_MIN guard", "random SPD"):
            assert not_ok == 0


def test_update_bit_equal_to_one_lane_update(output):
    m = re.search(r"update: (\d+) cases \((\d+) of them the systems above\), (\d+) differ; theta < 1e-6: (\d+), "
                  r"theta\^2 < 1e-6: (\d+), larger: (\d+); converged flag set in (\d+)", output)
    assert m, output
    cases, systems, differ, small, mid, large, conv = map(int, m.groups())
    assert systems == sum(GROUPS.values()) and cases > systems + 1000 and differ == 0
    assert small >= 100 and mid >= 100 and large >= 100  # both sides of the theta branch of se3_exp and of so3_exp
    assert 100 <= conv <= cases - systems - 100  # the criteria cases set the flag and leave it clear


def test_inputs_tell_a_reordered_back_substitution_apart(output):
    m = re.search(r"reordered back substitution \(descending j\) differs on (\d+) of (\d+) random systems", output)
    assert m, output
    differs, n = map(int, m.groups())
    assert n == 2000 and differs >= n // 2
