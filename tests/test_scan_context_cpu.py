"""Scan Context place recognition (csrc/place_recognition.hip) without a GPU: the symbols, the sector table, the host twin of the
descriptor against the float32 model of tests/f64_scan_context.py bit for bit, the guesses, the argument errors that need no
device, the compiler's resource report of the unit, and the condition the GPU end-to-end test rests on: on the model alone the
bundled target is the nearest entry to the source turned by 150 degrees, by more than 0.1, at shift 25."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import f64_scan_context as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("sp_scan_context_boundaries_host", "sp_scan_context_compute", "sp_scan_context_compute_host", "sp_scan_context_db_create",
           "sp_scan_context_db_destroy", "sp_scan_context_db_size", "sp_scan_context_db_clear", "sp_scan_context_db_add",
           "sp_scan_context_db_search_workspace_bytes", "sp_scan_context_db_search", "sp_scan_context_guesses_host")
CASES = model.descriptor_cases()


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def c_params(p):
    from sycl_points_amd import _lib

    return _lib.ScanContextParams(p["rings"], p["sectors"], p["max_range"], p["sensor_height"])


def test_symbols_and_abi(L):
    from sycl_points_amd import _lib

    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES, s
    assert L.sp_abi_version() == 7
    assert (_lib.SCAN_CONTEXT_MAX_K, _lib.SCAN_CONTEXT_DB_MAX) == (32, 1 << 20)
    import sycl_points_amd.api as sp

    for name in ("ScanContextParams", "scan_context", "ScanContextDatabase", "scan_context_guesses", "LoopCandidate"):
        assert hasattr(sp, name), name
    p = sp.ScanContextParams()
    assert (p.rings, p.sectors, p.max_range, p.sensor_height) == (20, 60, 80.0, 2.0)


@pytest.mark.parametrize("sectors", [4, 30, 60, 64])
def test_boundaries_are_the_models(L, sectors):
    c, s = np.full(64, np.nan, np.float32), np.full(64, np.nan, np.float32)
    assert L.sp_scan_context_boundaries_host(sectors, vp(c), vp(s)) == 0
    mc, ms = model.boundaries(sectors)
    assert np.array_equal(c[:sectors].view(np.uint32), mc.view(np.uint32))
    assert np.array_equal(s[:sectors].view(np.uint32), ms.view(np.uint32))
    assert np.isnan(c[sectors:]).all() and np.isnan(s[sectors:]).all()
    assert c[0] == -1.0 and c[sectors // 2] == 1.0 and abs(s[sectors // 2]) < 1e-15  # phi_0 = -pi, phi_h = 0 up to double rounding


def host_descriptor(L, p, points):
    P = np.ascontiguousarray(points, np.float32)
    out = np.full((p["rings"], p["sectors"]), np.nan, np.float32)
    prm = c_params(p)
    assert L.sp_scan_context_compute_host(C.byref(prm), vp(P), len(P), vp(out)) == 0
    return out


@pytest.mark.parametrize("name,p,points", CASES, ids=[c[0] for c in CASES])
def test_host_descriptor_is_the_models_bit_for_bit(L, name, p, points):
    got = host_descriptor(L, p, points)
    want = model.descriptor(points, p)
    kept = model.bins(points, p)[0]
    print(f"\n[scan context host {name}] {len(points)} points, {int(kept.sum())} kept, {int((want > 0).sum())} of {want.size} bins occupied")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    if name == "contention":
        assert (want > 0).sum() == 1 and kept.all()
    if name == "skipped":
        assert not kept[:37].any() and kept[37] and model.bins(points, p)[1][37] == p["rings"] - 1
    if name == "negative_values":
        assert (want == 0).all() or want.max() < 1.0
    if name.startswith("boundaries"):
        assert kept.sum() < len(points)  # the points at r = 0 and r = max_range


def test_empty_cloud_gives_zeros(L):
    p = model.params()
    prm = c_params(p)
    out = np.full((20, 60), np.nan, np.float32)
    assert L.sp_scan_context_compute_host(C.byref(prm), None, 0, vp(out)) == 0
    assert not out.any()


def test_sectors_follow_the_angle(L):
    """Away from the boundaries the count of half-plane tests is floor((atan2(y, x) + pi) / (2 pi / sectors))."""
    p = model.params()
    rs = np.random.RandomState(4)
    ang = rs.uniform(-np.pi, np.pi, 5000)
    P = np.ones((5000, 4), np.float32)
    P[:, 0], P[:, 1], P[:, 2] = 30.0 * np.cos(ang), 30.0 * np.sin(ang), 1.0
    frac = (np.arctan2(P[:, 1].astype(np.float64), P[:, 0].astype(np.float64)) + np.pi) / (2 * np.pi / 60)
    clear = np.abs(frac - np.round(frac)) > 1e-3
    _, ring, sector, _ = model.bins(P, p)
    assert np.array_equal(sector[clear], np.floor(frac[clear]).astype(np.int64) % 60) and (ring == 7).all()


@pytest.mark.parametrize("sectors,shift,steps", [(60, 25, 5), (60, 0, 1), (4, 3, 2), (64, 63, 7), (30, 14, 4)])
def test_guesses_are_the_models(L, sectors, shift, steps):
    prm = c_params(model.params(20, sectors))
    out = np.full((steps, 16), np.nan)
    assert L.sp_scan_context_guesses_host(C.byref(prm), shift, steps, vp(out)) == 0
    got = out.reshape(steps, 4, 4).transpose(0, 2, 1)  # column-major
    want = model.guesses(sectors, shift, steps)
    assert np.abs(got - want).max() <= 1e-15
    assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (steps, 1))) and not got[:, :3, 3].any()
    if steps % 2 == 1:  # delta = 0 is among them: exactly Rz(-shift 2 pi / sectors)
        mid = got[steps // 2]
        a = -shift * 2.0 * np.pi / sectors
        assert abs(mid[0, 0] - np.cos(a)) <= 1e-15 and abs(mid[1, 0] - np.sin(a)) <= 1e-15


def test_guess_sign_convention(L):
    """A scan turned by +s sectors has shift s against the original, and the guess Rz(-s 2 pi / sectors) takes its points back."""
    p = model.params()
    P = model.scan(20000, 11)
    s = 7
    turned = P.copy()
    turned[:, :3] = (P[:, :3].astype(np.float64) @ model.rot_z(s * 6.0)[:3, :3].T).astype(np.float32)
    d, shift = model.distance(model.descriptor(turned, p), model.descriptor(P, p))
    assert shift == s and d < 0.05, (d, shift)
    prm = c_params(p)
    out = np.zeros(16)
    assert L.sp_scan_context_guesses_host(C.byref(prm), shift, 1, vp(out)) == 0
    T = out.reshape(4, 4).T
    back = turned[:, :3].astype(np.float64) @ T[:3, :3].T
    assert np.abs(back - P[:, :3]).max() < 1e-4


def test_argument_errors_need_no_device(L):
    from sycl_points_amd import _lib

    bad = _lib.SP_ERR_INVALID_ARGUMENT
    p = C.c_void_p(4096)
    big = 1 << 40
    good = model.params()
    out = np.zeros((32, 64), np.float32)
    pts = np.ones((4, 4), np.float32)
    wrong = [dict(rings=0), dict(rings=33), dict(sectors=2), dict(sectors=66), dict(sectors=31), dict(max_range=0.0),
             dict(max_range=-1.0), dict(max_range=np.inf), dict(max_range=np.nan)]
    for w in wrong:
        prm = c_params({**good, **w})
        h = C.c_void_p(1)
        assert L.sp_scan_context_compute_host(C.byref(prm), vp(pts), 4, vp(out)) == bad, w
        assert L.sp_scan_context_compute(C.byref(prm), p, 4, p, None) == bad, w
        assert L.sp_scan_context_db_create(C.byref(prm), 0, C.byref(h)) == bad and not h.value, w
        assert L.sp_scan_context_guesses_host(C.byref(prm), 0, 1, vp(np.zeros(16))) == bad, w
    assert b"max_range" in L.sp_last_error()
    for sectors in (2, 3, 66):
        assert L.sp_scan_context_boundaries_host(sectors, vp(out), vp(out)) == bad
    assert L.sp_scan_context_boundaries_host(60, None, vp(out)) == bad
    prm = c_params(good)
    assert L.sp_scan_context_compute_host(None, vp(pts), 4, vp(out)) == bad
    assert L.sp_scan_context_compute_host(C.byref(prm), None, 4, vp(out)) == bad
    assert L.sp_scan_context_compute_host(C.byref(prm), vp(pts), 4, None) == bad
    assert L.sp_scan_context_compute(C.byref(prm), None, 4, p, None) == bad
    assert L.sp_scan_context_compute(C.byref(prm), p, 4, None, None) == bad
    assert L.sp_scan_context_compute(C.byref(prm), p, 1 << 32, p, None) == bad
    assert L.sp_scan_context_guesses_host(C.byref(prm), 60, 1, vp(np.zeros(16))) == bad
    assert L.sp_scan_context_guesses_host(C.byref(prm), 3, 2, None) == bad
    assert L.sp_scan_context_guesses_host(C.byref(prm), 3, 0, None) == 0
    # the database: creating, asking and destroying one takes no device
    h = C.c_void_p()
    assert L.sp_scan_context_db_create(C.byref(prm), (1 << 20) + 1, C.byref(h)) == bad
    assert L.sp_scan_context_db_create(C.byref(prm), 16, None) == bad
    assert L.sp_scan_context_db_create(C.byref(prm), 16, C.byref(h)) == 0 and h.value
    try:
        assert L.sp_scan_context_db_size(h) == 0 and L.sp_scan_context_db_clear(h) == 0
        assert L.sp_scan_context_db_add(h, None, None) == bad
        assert L.sp_scan_context_db_add(None, p, None) == bad
        need = L.sp_scan_context_db_search_workspace_bytes(h, 1000)
        assert need >= 20 * 64 * 4 + 9 * 1000  # the query as an entry, a key and a shift per candidate
        assert L.sp_scan_context_db_search_workspace_bytes(None, 10) == 0
        assert L.sp_scan_context_db_search_workspace_bytes(h, (1 << 20) + 1) == 0
        # search(db, desc, first, count, k, idx, dist, shift, ws, ws_bytes, stream)
        assert L.sp_scan_context_db_search(None, p, 0, 0, 1, p, p, p, p, big, None) == bad
        assert L.sp_scan_context_db_search(h, p, 0, 0, 33, p, p, p, p, big, None) == bad and b"SP_SCAN_CONTEXT_MAX_K" in L.sp_last_error()
        assert L.sp_scan_context_db_search(h, p, 0, 1, 1, p, p, p, p, big, None) == bad and b"range" in L.sp_last_error()
        assert L.sp_scan_context_db_search(h, p, 1, 0, 1, p, p, p, p, big, None) == bad
        for hole in range(5):
            a = [p, p, p, p, p]
            a[hole] = None
            assert L.sp_scan_context_db_search(h, a[0], 0, 0, 4, a[1], a[2], a[3], a[4], big, None) == bad, hole
        small = L.sp_scan_context_db_search_workspace_bytes(h, 0)
        assert L.sp_scan_context_db_search(h, p, 0, 0, 4, p, p, p, p, small - 1, None) == bad and b"workspace" in L.sp_last_error()
        assert L.sp_scan_context_db_search(h, p, 0, 0, 4, p, p, p, C.c_void_p(4100), big, None) == bad
        assert L.sp_scan_context_db_search(h, None, 0, 0, 0, None, None, None, None, 0, None) == 0  # k == 0: nothing to do
    finally:
        L.sp_scan_context_db_destroy(h)
    L.sp_scan_context_db_destroy(None)
    assert L.sp_scan_context_db_clear(None) == bad and L.sp_scan_context_db_size(None) == 0


def test_no_kernel_of_the_unit_uses_scratch(L):
    rows = [l for l in open(os.path.join(ROOT, "sycl_points_amd", "lib", "place_recognition.resources.txt")) if "Function Name" in l]
    names = " ".join(rows)
    for kernel in ("descriptor_kernel", "normalise_kernel", "search_kernel", "select_kernel"):
        assert kernel in names, kernel
    assert len([r for r in rows if "search_kernel" in r]) == 16  # KS = 2 .. 16, one and two tiles
    for row in rows:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", row).group(1)) == 0, row
        assert int(re.search(r"VGPRs Spill: (\d+)", row).group(1)) == 0, row


def test_the_model_recognises_the_bundled_pair():
    """Defaults, raw bundled scans, the source turned by 150 degrees: the target's distance is the smallest, smaller by more than
    0.1 than every decoy's, at shift 25 = 150 / 6 (recorded: 0.106 against >= 0.30)."""
    p = model.params()
    query, entries = model.bundled_clouds(GOLD)
    Q = model.descriptor(query, p)
    found = [model.distance(Q, model.descriptor(e, p)) for e in entries]
    print(f"\n[scan context, model] {int((Q > 0).sum())} of {Q.size} bins occupied; (distance, shift) against random, scaled, target, "
          f"mirrored: {[(round(d, 4), s) for d, s in found]}")
    d_target, shift = found[2]
    assert shift == 25
    for i in (0, 1, 3):
        assert found[i][0] > d_target + 0.1, (i, found)
