"""The wave form of the iteration finish on the device (csrc/sp_wave_solve.h through sp_internal_finish_wave: one wave per case, as
wave 0 of the alignment kernels runs it) against the one-lane code it replaces, bit for bit, on the cases of
tests/cpp/test_wave_solve.cpp (--dump: every pivot order, ties, zero pivots, the FLT_MIN guard, 1e-30 / 1e30, NaN / inf, 2000 random
SPD systems, steps from 1e-9 to 4 rad on both sides of the theta branches, criteria one ulp either side of |delta|):
  T, delta8   against the device's one-lane sp_gn_update (device sinf / cosf on both sides — the comparison that matters; a pose is
              never compared across host and device),
  x           against sp_ldlt6_solve_host of (H + lambda I, -b): +, -, *, / only, correctly rounded on both sides."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from test_wave_solve_cpu import build_program

pytestmark = pytest.mark.gpu

f32 = np.float32


def differing_rows(a, b):
    """Rows in which a word differs in its bits — except NaN against NaN: IEEE 754 leaves a NaN result's sign and payload open, and the
    two code paths may meet the operands of a sum in either order (tests/cpp/test_wave_solve.cpp, same_bits)."""
    d = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    return np.flatnonzero(d.any(axis=1))


def tri(a, c):
    return a * 6 - a * (a - 1) // 2 + (c - a)


TRI = np.array([[tri(min(a, c), max(a, c)) for c in range(6)] for a in range(6)])


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("wave_solve_gpu")
    exe = build_program(str(d / "test_wave_solve"), "-O2")
    dump = str(d / "cases.bin")
    r = subprocess.run([exe, "--dump", dump], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    c = np.fromfile(dump, dtype=f32).reshape(-1, 49)
    assert c.shape[0] > 4000
    return {"tot": np.ascontiguousarray(c[:, :30]), "T": np.ascontiguousarray(c[:, 30:46]), "par": np.ascontiguousarray(c[:, 46:49])}


@pytest.fixture(scope="module")
def wave(sp, cases):
    """One launch: every case through the wave form."""
    n = cases["tot"].shape[0]
    dev = lambda a: torch.from_numpy(a.copy()).cuda()  # noqa: E731
    tot, par, T = dev(cases["tot"]), dev(cases["par"]), dev(cases["T"])
    d8 = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda")
    x = torch.full((n, 6), 7.0, dtype=torch.float32, device="cuda")
    sp.check(sp._lib.lib().sp_internal_finish_wave(sp._ptr(tot), sp._ptr(par), sp._ptr(T), sp._ptr(d8), sp._ptr(x), n, sp._stream()))
    torch.cuda.synchronize()
    return {"T": T.cpu().numpy(), "d8": d8.cpu().numpy(), "x": x.cpu().numpy()}


def linearized_words(tot):
    """sp_linearized (48 words) of every case: H symmetric from the 21 totals, b, error; the count folds to 0."""
    n = tot.shape[0]
    lin = np.zeros((n, 48), f32)
    lin[:, :36] = tot[:, TRI.reshape(-1)]
    lin[:, 36:42] = tot[:, 21:27]
    lin[:, 42] = tot[:, 27]
    return lin


def test_pose_and_delta_bit_equal_to_one_lane_device_update(sp, cases, wave):
    n = cases["tot"].shape[0]
    lin = torch.from_numpy(linearized_words(cases["tot"])).cuda()
    T = torch.from_numpy(cases["T"].copy()).cuda()
    d8 = torch.full((n, 8), 9.0, dtype=torch.float32, device="cuda")
    L = sp._lib.lib()
    par = cases["par"]
    for i in range(n):
        sp.check(L.sp_gn_update(sp._ptr(lin[i]), sp._ptr(T[i]), float(par[i, 0]), float(par[i, 1]), float(par[i, 2]), sp._ptr(d8[i]),
                                sp._stream()))
    torch.cuda.synchronize()
    T1, d1 = T.cpu().numpy(), d8.cpu().numpy()
    bad_T = differing_rows(T1, wave["T"])
    bad_d = differing_rows(d1, wave["d8"])
    print(f"{n} cases: pose differs in {bad_T.size}, delta8 in {bad_d.size}; converged set in {int((d1[:, 6] > 0.5).sum())}, "
          f"not ok in {int((d1[:, 7] < 0.5).sum())}")
    assert bad_d.size == 0, (bad_d[:10], d1[bad_d[:3]], wave["d8"][bad_d[:3]])
    assert bad_T.size == 0, (bad_T[:10], T1[bad_T[:3]], wave["T"][bad_T[:3]])
    assert (d1[:, 6] > 0.5).sum() > 100 and (d1[:, 7] < 0.5).sum() >= 15  # both flags are exercised


def test_raw_solution_bit_equal_to_host_solver(sp, cases, wave):
    L = sp._lib.lib()
    tot, par = cases["tot"], cases["par"]
    n = tot.shape[0]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    x = np.zeros((n, 6), f32)
    ok = np.zeros(n, bool)
    for i in range(n):
        H = np.ascontiguousarray(tot[i, TRI])
        H[np.arange(6), np.arange(6)] = H[np.arange(6), np.arange(6)] + par[i, 0] * f32(1.0)
        rhs = -tot[i, 21:27]
        ok[i] = L.sp_ldlt6_solve_host(vp(H), vp(rhs), vp(x[i])) == 0
    bad = differing_rows(x, wave["x"])
    print(f"{n} systems: x differs in {bad.size}; not ok in {int((~ok).sum())}")
    assert bad.size == 0, (bad[:10], x[bad[:3]], wave["x"][bad[:3]])
    assert np.array_equal(wave["d8"][:, 7] > 0.5, ok)
    assert differing_rows(wave["d8"][:, :6], wave["x"]).size == 0  # delta IS the raw solution
