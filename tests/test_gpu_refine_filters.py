"""The scan filters that follow kNN and covariances on the device (sp_angle_incidence_flags, sp_intensity_correct,
sp_intensity_gaussian, their Python mirror and, through tests/cpp/test_refine_filters.cpp, the C++ facade) against the CPU
restatement of the four formulas (tests/cpp/refine_restate.cpp).

Clouds: 20 001 points on three noisy planes (more than one workgroup, a grid-stride tail, no multiple of 64 or 256), neighbours
from the library's KDTree (k = 10), covariances and normals from the library, intensities U[0, 255), and the planted rows of
tests/test_refine_filters_cpu.py (a NaN point, an Inf point, a zero normal, the origin, the zenith, neighbours out of reach,
indices outside [0, n)); N = 0, 1 and 7 (kNN of 7 points with k = 10 carries -1 padding); index rows of stride 20, 10 and 3.

Angle of incidence: the flags are the restatement's bit for bit — the formula is fma chains, two square roots, one product, one
division and comparisons, all correctly rounded on both sides (the library is built without fast-math; hipcc rounds sqrt and
division correctly by default) — and the covariance path's flags are the normal path's on sp_normals_from_cov's output bit for
bit, because both call one normal_of (csrc/sp_cov_normal.h). No band, no excluded rows.

Intensities: a float64 evaluation of the same formula is the yardstick. E_ref is the float32 restatement's largest absolute
error against it, E_dev the device's, and the device passes when E_dev <= m * E_ref, with tests/test_gpu_deskew.py's rule for m:
the OpenCL full-profile bound of the least accurate device function in the formula over glibc's 1 ulp, times 2 for the spread
between two samples' worst rows. The correction's least accurate function is pow (16 ulp): m = 32. The Gaussian's is exp
(3 ulp): m = 6. The sigmas keep the largest exponent of the regular rows below 80 (asserted), so no weight is denormal.
m, E_ref and E_dev are printed before every assertion (run with -s).

Measured on an MI355X: 0 of 20 001 flags differ in each band; correction E_dev / E_ref = 1.14e-4 / 1.14e-4 (distance), 1.26e-4 /
1.19e-4 (normals and covs); smoothing 6.5e-5 / 6.7e-5 (stride 10 and 20), 3.4e-5 / 4.0e-5 (stride 3); normalisation 6.3e-7 /
6.5e-7 and 4.1e-7 / 3.7e-7; the largest exponent of the regular rows is 25.9.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
N, K = 20001, 10
M_POW, M_EXP = 32.0, 6.0  # (16 ulp pow | 3 ulp exp over 1 ulp glibc) x 2
SIGMAS = (0.1, 0.1, 0.05)
HALF_PI = float(np.float32(np.pi) * np.float32(0.5))


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def cpu():
    import importlib.util

    spec = importlib.util.spec_from_file_location("refine_cpu_helpers", os.path.join(ROOT, "tests", "test_refine_filters_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def R(cpu, tmp_path_factory):
    return cpu.build_restatement(tmp_path_factory.mktemp("refine"))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else _vp(t.data_ptr())


def stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def lib():
    from sycl_points_amd import _lib

    return _lib.lib()


def library_attributes(sp, pts, k):
    """(knn, covs, normals) of a clean cloud through the library: KDTree, covariance.estimate, extract_normals"""
    P = dev(pts)
    knn = sp.KDTree.build(P).knn_search(P, k).indices
    covs = sp.covariance.estimate(knn, P)
    nrm = sp.covariance.extract_normals(P, covs)
    torch.cuda.synchronize()
    return knn.cpu().numpy(), covs.cpu().numpy(), nrm.cpu().numpy()


@pytest.fixture(scope="module")
def scene(sp, cpu):
    pts, inten, stamps = cpu.planes_cloud(N)
    knn, covs, _ = library_attributes(sp, pts, K)
    assert knn.shape == (N, K) and knn.min() >= 0
    pts, _, covs, knn, regular = cpu.plant_rows(pts, np.zeros((N, 4), np.float32), covs, knn)
    nrm_lib = sp.covariance.extract_normals(dev(pts), dev(covs)).cpu().numpy()  # what the covariance paths must reproduce
    nrm = nrm_lib.copy()
    nrm[cpu.PLANTED["zero_normal"]] = 0.0
    return dict(pts=pts, inten=inten, stamps=stamps, knn=knn, covs=covs, nrm=nrm, nrm_lib=nrm_lib, regular=regular)


def device_flags(pts, nrm, covs, lo, hi):
    n = len(pts)
    flags = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    P, Nr, Cv = dev(pts), dev(nrm), dev(covs)  # (named: the tensors must outlive the launch)
    rc = lib().sp_angle_incidence_flags(ptr(P), ptr(Nr), ptr(Cv), n, lo, hi, ptr(flags), stream())
    assert rc == 0, lib().sp_last_error()
    torch.cuda.synchronize()
    return flags.cpu().numpy()[:n]


def device_correct(pts, nrm, covs, inten, exponent=2.0, scale=1.0, lo=0.0, hi=1000.0, ref=1.0, angle_exponent=0.0):
    I, P, Nr, Cv = dev(inten), dev(pts), dev(nrm), dev(covs)
    rc = lib().sp_intensity_correct(ptr(P), ptr(Nr), ptr(Cv), ptr(I), len(pts), exponent, scale, lo, hi, ref,
                                    angle_exponent, stream())
    assert rc == 0, lib().sp_last_error()
    torch.cuda.synchronize()
    return I.cpu().numpy()


def device_gaussian(pts, inten, knn, sigmas=SIGMAS, mean_min=0.0, k_limit=0):
    n, k = knn.shape
    k_use = k_limit if 0 < k_limit < k else k
    out = torch.full((max(n, 1),), -5.0, dtype=torch.float32, device="cuda")
    P, I, Kn = dev(pts), dev(inten), dev(np.ascontiguousarray(knn, np.int32))
    rc = lib().sp_intensity_gaussian(ptr(P), ptr(I), ptr(Kn), n, k, k_use, *sigmas,
                                     mean_min, ptr(out), stream())
    assert rc == 0, lib().sp_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()[:n]


def small_scene(sp, cpu, n):
    pts, inten, stamps = cpu.planes_cloud(n, seed=77)
    knn, covs, nrm = library_attributes(sp, pts, K)
    return pts, inten, stamps, knn, covs, nrm


# ------------------------------------------------------------------------------------------------ angle of incidence
@pytest.mark.parametrize("band", [(0.2, 1.2), (0.0, HALF_PI), (0.6, 0.9)])
def test_angle_flags_normals_bit_for_bit(cpu, R, scene, band):
    """sp_angle_incidence_flags with normals: the restatement's flags, every row (see the module docstring for why exactly)"""
    want = cpu.angle_flags(R, scene["pts"], scene["nrm"], *band)
    got = device_flags(scene["pts"], scene["nrm"], None, *band)
    print(f"angle flags {band}: kept {int(got.sum())} of {N}, differing rows {int((got != want).sum())}")
    assert np.array_equal(got, want)
    for name in ("nan", "inf", "zero_normal", "origin"):
        assert got[cpu.PLANTED[name]] == 0, name
    assert 0 < got.sum() < N


def test_angle_flags_covs_equal_normals_path(cpu, scene):
    """the covariance path decides as the normal path does on sp_normals_from_cov's output: one normal_of, the same bits"""
    for band in ((0.2, 1.2), (0.0, HALF_PI), (0.6, 0.9)):
        a = device_flags(scene["pts"], None, scene["covs"], *band)
        b = device_flags(scene["pts"], scene["nrm_lib"], None, *band)
        assert np.array_equal(a, b), band
        # normals win when both are given
        assert np.array_equal(device_flags(scene["pts"], scene["nrm"], scene["covs"], *band), device_flags(scene["pts"], scene["nrm"], None, *band))


def test_angle_filter_compacts_every_attribute(sp, cpu, R, scene):
    """api.angle_incidence_filter: the kept count and every attribute are numpy's compaction by the restatement's flags, byte for
    byte; the source is left alone (the C++ facade's in-place form is tests/cpp/test_refine_filters.cpp's)"""
    attrs = dict(covs=scene["covs"], normals=scene["nrm"], intensities=scene["inten"], timestamp_offsets=scene["stamps"])
    pc = sp.PointCloudShared.from_numpy(scene["pts"], **attrs)
    out, flags = sp.angle_incidence_filter(pc, 0.2, 1.2, return_flags=True)
    want = cpu.angle_flags(R, scene["pts"], scene["nrm"], 0.2, 1.2).astype(bool)
    assert np.array_equal(flags.cpu().numpy().astype(bool), want)
    assert out.size() == int(want.sum())
    for name, src in dict(points=scene["pts"], **attrs).items():
        got = getattr(out, name).cpu().numpy()
        assert got.tobytes() == np.ascontiguousarray(src[want]).tobytes(), name
        assert getattr(pc, name).cpu().numpy().tobytes() == src.tobytes(), name
    # covariances alone select the normals of the covariances
    pc2 = sp.PointCloudShared.from_numpy(scene["pts"], covs=scene["covs"], intensities=scene["inten"])
    out2 = sp.angle_incidence_filter(pc2, 0.2, 1.2)
    want2 = cpu.angle_flags(R, scene["pts"], scene["nrm_lib"], 0.2, 1.2).astype(bool)
    assert out2.points.cpu().numpy().tobytes() == np.ascontiguousarray(scene["pts"][want2]).tobytes()
    assert out2.normals is None and out2.intensities.cpu().numpy().tobytes() == scene["inten"][want2].tobytes()
    # the reference's errors, and the empty cloud that returns before them
    from sycl_points_amd._lib import SpError

    with pytest.raises(SpError, match="must be pre-computed"):
        sp.angle_incidence_filter(sp.PointCloudShared.from_numpy(scene["pts"]), 0.2, 1.2)
    with pytest.raises(SpError, match="Invalid angle range"):
        sp.angle_incidence_filter(pc, 1.2, 0.2)
    empty = sp.PointCloudShared()
    assert sp.angle_incidence_filter(empty, 1.2, 0.2) is empty


@pytest.mark.parametrize("n", [1, 7])
def test_small_clouds(sp, cpu, R, n):
    """one point and seven (their kNN rows carry -1 padding): every kernel against the restatement. A handful of rows can by
    chance all round exactly, which says nothing about float32: here E_ref is taken to be at least the final rounding the
    restatement can commit, half an ulp of the largest result."""
    def e_ref(r32, r64):
        return max(float(np.abs(r32 - r64).max()), 0.5 * float(np.spacing(np.float32(np.abs(r64).max()))))

    pts, inten, stamps, knn, covs, nrm = small_scene(sp, cpu, n)
    assert knn.shape == (n, K) and (knn[:, n:] == -1).all() and (knn[:, :n] >= 0).all()
    assert np.array_equal(device_flags(pts, nrm, None, 0.0, HALF_PI), cpu.angle_flags(R, pts, nrm, 0.0, HALF_PI))
    assert np.array_equal(device_flags(pts, None, covs, 0.0, HALF_PI), device_flags(pts, nrm, None, 0.0, HALF_PI))
    for fn_kw in (dict(), dict(mean_min=1e-3)):
        ref64 = cpu.gaussian(R, pts, inten, knn, *SIGMAS, f64=True, **fn_kw)
        E_ref = e_ref(cpu.gaussian(R, pts, inten, knn, *SIGMAS, **fn_kw), ref64)
        E_dev = float(np.abs(device_gaussian(pts, inten, knn, **fn_kw) - ref64).max())
        print(f"small cloud n = {n} {fn_kw}: E_dev = {E_dev:.3e}  E_ref = {E_ref:.3e}  m = {M_EXP}")
        assert E_dev <= M_EXP * E_ref
    ref64 = cpu.correct(R, pts, nrm, inten, 2.0, 1.0, 0.0, 1e6, 1.0, 1.0, f64=True)
    E_ref = e_ref(cpu.correct(R, pts, nrm, inten, 2.0, 1.0, 0.0, 1e6, 1.0, 1.0), ref64)
    E_dev = float(np.abs(device_correct(pts, nrm, None, inten, 2.0, 1.0, 0.0, 1e6, 1.0, 1.0) - ref64).max())
    print(f"small cloud n = {n} correction: E_dev = {E_dev:.3e}  E_ref = {E_ref:.3e}  m = {M_POW}")
    assert E_dev <= M_POW * E_ref


def test_empty_cloud_enqueues_nothing(sp):
    """n = 0: SP_OK from every entry point (null pointers, no launch) and the Python mirror leaves the cloud alone"""
    L = lib()
    assert L.sp_angle_incidence_flags(None, None, None, 0, 0.2, 1.2, None, stream()) == 0
    assert L.sp_intensity_correct(None, None, None, None, 0, 2.0, 1.0, 0.0, 1000.0, 1.0, 0.0, stream()) == 0
    assert L.sp_intensity_gaussian(None, None, None, 0, 10, 10, 0.1, 0.1, 0.05, 0.0, None, stream()) == 0
    empty = sp.PointCloudShared()
    sp.correct_intensity(empty, exponent=-1.0)
    sp.smooth_intensity(empty, sp.KNNResult(), 0.0, 0.0)
    sp.normalize_intensity_local_mean(empty, sp.KNNResult(), 0.1, 0.1, mean_min=-1.0)
    assert empty.size() == 0 and empty.intensities is None


# ------------------------------------------------------------------------------------------------ intensity correction
CORRECTION_CASES = {"distance": (False, False, 0.0), "normals": (True, False, 1.0), "covs": (False, True, 1.0)}


@pytest.mark.parametrize("case", list(CORRECTION_CASES))
def test_intensity_correction(cpu, R, scene, case):
    """E_dev <= 32 E_ref against float64 (pow: 16 ulp over glibc's 1, times 2), and the rows the yardstick clamps by more than that
    margin sit on the bound exactly"""
    with_n, with_c, ae = CORRECTION_CASES[case]
    pts, inten = scene["pts"], scene["inten"]
    nrm_dev = scene["nrm"] if with_n else None
    nrm_ref = scene["nrm"] if with_n else (scene["nrm_lib"] if with_c else None)
    covs = scene["covs"] if with_c else None
    finite = np.isfinite(pts).all(axis=1)
    lo, hi = 40.0, 400.0
    args = (1.7, 0.9, lo, hi, 1.3, ae)
    ref64 = cpu.correct(R, pts, nrm_ref, inten, *args, f64=True)
    free64 = cpu.correct(R, pts, nrm_ref, inten, 1.7, 0.9, -np.inf, np.inf, 1.3, ae, f64=True)
    ref32 = cpu.correct(R, pts, nrm_ref, inten, *args)
    got = device_correct(pts, nrm_dev, covs, inten, *args)
    E_ref = float(np.abs(ref32[finite] - ref64[finite]).max())
    E_dev = float(np.abs(got[finite] - ref64[finite]).max())
    print(f"intensity correction [{case}]: E_dev = {E_dev:.3e}  E_ref = {E_ref:.3e}  m = {M_POW}")
    assert E_ref > 0.0
    assert E_dev <= M_POW * E_ref
    above, below = finite & (free64 > hi + M_POW * E_ref), finite & (free64 < lo - M_POW * E_ref)
    assert above.sum() > 100 and below.sum() > 100
    assert (got[above] == np.float32(hi)).all() and (got[below] == np.float32(lo)).all()


def test_intensity_correction_exact_properties(cpu, scene):
    pts, inten, nrm, covs = scene["pts"], scene["inten"], scene["nrm"], scene["covs"]
    bits = cpu.bits
    # angle_exponent = 0 with normals (or covariances): the bits of the call without them, every row
    plain = device_correct(pts, None, None, inten, 2.0, 0.7, 0.0, 1000.0, 2.0, 0.0)
    assert np.array_equal(bits(device_correct(pts, nrm, None, inten, 2.0, 0.7, 0.0, 1000.0, 2.0, 0.0)), bits(plain))
    assert np.array_equal(bits(device_correct(pts, None, covs, inten, 2.0, 0.7, 0.0, 1000.0, 2.0, 0.0)), bits(plain))
    # exponent = 0: clamp(I * scale) exactly
    want = np.minimum(np.maximum(inten * np.float32(1.5), np.float32(10.0)), np.float32(300.0))
    assert np.array_equal(bits(device_correct(pts, None, None, inten, 0.0, 1.5, 10.0, 300.0)), bits(want))
    # the covariance path is the normal path on sp_normals_from_cov's output, bit for bit; normals win over covariances
    a = device_correct(pts, None, covs, inten, 2.0, 1.0, 0.0, 1e6, 1.0, 1.0)
    b = device_correct(pts, scene["nrm_lib"], None, inten, 2.0, 1.0, 0.0, 1e6, 1.0, 1.0)
    assert np.array_equal(bits(a), bits(b))
    c = device_correct(pts, nrm, covs, inten, 2.0, 1.0, 0.0, 1e6, 1.0, 1.0)
    assert np.array_equal(bits(c), bits(device_correct(pts, nrm, None, inten, 2.0, 1.0, 0.0, 1e6, 1.0, 1.0)))
    # a zero normal and the origin: angle factor 1
    none = device_correct(pts, None, None, inten, 2.0, 1.0, 0.0, 1e6, 1.0, 1.0)
    for name in ("zero_normal", "origin"):
        r = cpu.PLANTED[name]
        assert bits(c[r:r + 1])[0] == bits(none[r:r + 1])[0], name


# ------------------------------------------------------------------------------------------------ Gaussian smoothing, local mean
def wide_knn(knn, stride):
    """the rows of knn as the first K entries of rows `stride` wide (the rest: the row reversed, then -1)"""
    n, k = knn.shape
    out = np.full((n, stride), -1, np.int32)
    out[:, :k] = knn
    out[:, k:min(2 * k, stride)] = knn[:, ::-1][:, :max(0, min(2 * k, stride) - k)]
    return out


@pytest.mark.parametrize("mode", ["smooth", "normalize"])
def test_gaussian_against_float64(cpu, R, scene, mode):
    """E_dev <= 6 E_ref against float64 (exp: 3 ulp over glibc's 1, times 2) over the regular rows, the zenith rows and the rows
    with indices outside [0, n) (the restatement drops those neighbours too), for index rows of stride 10, 3 and 20 (k_limit 10)"""
    pts, inten, knn, regular = scene["pts"], scene["inten"], scene["knn"], scene["regular"]
    mean_min = 1e-3 if mode == "normalize" else 0.0
    rows = regular.copy()
    rows[list(cpu.PLANTED["zenith"]) + list(cpu.PLANTED["out_of_range"])] = True
    for label, table, k_limit in (("stride 10", knn, 0), ("stride 3", np.ascontiguousarray(knn[:, :3]), 0),
                                  ("stride 20, k_limit 10", wide_knn(knn, 20), 10)):
        ref32, _, emax = cpu.gaussian(R, pts, inten, table, *SIGMAS, mean_min=mean_min, k_limit=k_limit, exponents=True)
        ref64 = cpu.gaussian(R, pts, inten, table, *SIGMAS, mean_min=mean_min, k_limit=k_limit, f64=True)
        assert emax[regular].max() < 80.0, emax[regular].max()  # no denormal weight
        got = device_gaussian(pts, inten, table, mean_min=mean_min, k_limit=k_limit)
        E_ref = float(np.abs(ref32[rows] - ref64[rows]).max())
        E_dev = float(np.abs(got[rows] - ref64[rows]).max())
        print(f"gaussian [{mode}, {label}]: E_dev = {E_dev:.3e}  E_ref = {E_ref:.3e}  m = {M_EXP}  largest exponent = {emax[regular].max():.1f}")
        assert E_ref > 0.0
        assert E_dev <= M_EXP * E_ref
        for a in cpu.PLANTED["out_of_range"]:  # each such row on its own, within the same bound
            assert abs(float(got[a]) - ref64[a]) <= M_EXP * E_ref, a


def test_gaussian_exact_properties(cpu, R, scene):
    pts, inten, knn, regular = scene["pts"], scene["inten"], scene["knn"], scene["regular"]
    bits = cpu.bits
    out = device_gaussian(pts, inten, knn)
    # every listed neighbour has an exponent above 200 and the row does not list itself: the own intensity, unchanged
    far = cpu.PLANTED["far"]
    _, emin, _ = cpu.gaussian(R, pts, inten, knn, *SIGMAS, exponents=True)
    assert emin[far] > 200.0 and far not in knn[far]
    assert bits(out[far:far + 1])[0] == bits(inten[far:far + 1])[0]
    org = cpu.PLANTED["origin"]
    assert bits(out[org:org + 1])[0] == bits(inten[org:org + 1])[0]
    z = list(cpu.PLANTED["zenith"])
    assert np.isfinite(out[z]).all() and out[z].min() >= inten[z].min() and out[z].max() <= inten[z].max()
    # k_limit 10 on a stride-20 result (16-byte rows) is the stride-10 prefix array's result (dword rows), bit for bit
    assert np.array_equal(bits(device_gaussian(pts, inten, wide_knn(knn, 20), k_limit=10)), bits(out))
    assert np.array_equal(bits(device_gaussian(pts, inten, wide_knn(knn, 12), k_limit=10)), bits(out))
    assert np.array_equal(bits(device_gaussian(pts, inten, knn, k_limit=3)), bits(device_gaussian(pts, inten, np.ascontiguousarray(knn[:, :3]))))
    # local-mean normalisation: flat intensity gives 1 within the reference's own tolerance; zero intensity hits the clamp: exactly 0
    flat = device_gaussian(pts, np.full(N, 37.5, np.float32), knn, mean_min=1e-3)
    assert np.abs(flat[regular] - 1.0).max() <= 1e-4
    zero = device_gaussian(pts, np.zeros(N, np.float32), knn, mean_min=1e-3)
    assert not bits(zero[regular]).any()
    assert np.array_equal(bits(device_gaussian(pts, inten, wide_knn(knn, 20), mean_min=1e-3, k_limit=10)),
                          bits(device_gaussian(pts, inten, knn, mean_min=1e-3)))


def test_python_mirror(sp, cpu, scene):
    """api.correct_intensity / smooth_intensity / normalize_intensity_local_mean are the C calls; the latter two swap a fresh
    tensor in; the reference's errors come through"""
    from sycl_points_amd._lib import SpError

    pts, inten, knn, nrm = scene["pts"], scene["inten"], scene["knn"], scene["nrm"]
    bits = cpu.bits
    pc = sp.PointCloudShared.from_numpy(pts, normals=nrm, intensities=inten)
    before = pc.intensities
    sp.correct_intensity(pc, 2.0, 0.5, 0.0, 500.0, 1.5, 1.0)
    assert pc.intensities is before
    c = device_correct(pts, nrm, None, inten, 2.0, 0.5, 0.0, 500.0, 1.5, 1.0)
    assert np.array_equal(bits(pc.intensities.cpu().numpy()), bits(c))
    res = sp.KNNResult(indices=dev(wide_knn(knn, 20)), query_size=N, k=20)
    sp.smooth_intensity(pc, res, *SIGMAS, k_limit=10)
    assert pc.intensities is not before
    s = device_gaussian(pts, c, knn)
    assert np.array_equal(bits(pc.intensities.cpu().numpy()), bits(s))
    sp.normalize_intensity_local_mean(pc, res, *SIGMAS, k_limit=10)
    assert np.array_equal(bits(pc.intensities.cpu().numpy()), bits(device_gaussian(pts, s, knn, mean_min=1e-3)))
    with pytest.raises(SpError, match=r"\[correct_intensity\] ref_distance must be positive"):
        sp.correct_intensity(pc, ref_distance=0.0)
    with pytest.raises(SpError, match=r"\[correct_intensity\] Intensity field not found"):
        sp.correct_intensity(sp.PointCloudShared.from_numpy(pts))
    with pytest.raises(SpError, match=r"\[intensity_gaussian::smooth_intensity\] All sigma values must be positive"):
        sp.smooth_intensity(pc, res, 0.0, 0.1)
    with pytest.raises(SpError, match=r"\[intensity_local_mean_norm::normalize\] mean_min must be positive"):
        sp.normalize_intensity_local_mean(pc, res, 0.1, 0.1, mean_min=0.0)
    with pytest.raises(SpError, match=r"\[intensity_local_mean_norm::normalize\] Intensity field not found"):
        sp.normalize_intensity_local_mean(sp.PointCloudShared.from_numpy(pts), res, 0.1, 0.1, mean_min=0.0)


def test_cpp_facade(sp, R):
    """tests/cpp/test_refine_filters.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed): the
    four facade functions against the restatement on the 20 001-point cloud and the small shapes, the reference's exception cases,
    in-place and out-of-place angle filtering, and the refine_filter order end to end on tests/golden/source.ply."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_refine_filters")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{rocm}/include",
                           "-D__HIP_PLATFORM_AMD__", "-Wall", "-Wno-unused-value", "-Wno-unused-result",
                           os.path.join(cpp, "test_refine_filters.cpp"), "-o", exe, f"-L{libdir}", "-lsycl_points_amd",
                           f"-Wl,-rpath,{libdir}", f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "source.ply")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
