"""The first trip of a gicp_align_kernel launch takes its pose-independent loads (the point's three coordinate words, its
48-byte correspondence row) from registers that were filled inside the prologue (csrc/registration.hip, PointHead in
csrc/registration_device.h). What can go wrong is a wrong point (the tile / lane arithmetic of i0, a lane without a point), a
wrong or stale row, a first trip that is taken twice or not at all, and a launch that ends in its prologue.

  * per launch: four launches of sp_gicp_align_step from a pose one target cell off the truth, so that launches 1-3 mix
    certified and searched points. Every point's neighbour is the one an independent search (GridKNN's external k = 1 query,
    another kernel, held to brute force by test_gpu_parity.py) finds for T_k p — a wrong prefetched POINT breaks this — and
    distances, partial rows, linear system and state are the bytes of the same launches with reuse = 0, where no row is read
    and every point is searched — a wrong or stale prefetched ROW breaks this;
  * whole alignments (default criteria: launches that converge in their prologue and return with the loads outstanding;
    criteria 0 and 6 iterations) are the bytes of reuse = 0, repeat bit for bit, and land on the generic loop's pose.

Sizes: the guard on lanes without a point (1, 1023), one full workgroup (1024), a second workgroup with one live lane (1025),
256 workgroups whose every lane makes exactly one — prefetched — trip (262144), exactly one lane with a second trip (262145),
a full row of second trips plus one (263169).

NOT compared between reuse on and off, although both belong to the state: the searched-point count. It is n with reuse = 0
by definition and smaller with reuse on; it is held to n on the one side and to [0, n] on the other.
The source's tiles are filled with NaN before the preparation (the unused lanes of the last tile stay NaN); the cache rows have
no entry point that reaches them from here, they start as the allocator left them.
"""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_TARGET = 3000
NS = [1, 1023, 1024, 1025, 262144, 262145, 263169]
N_MAX = max(NS)
BOTH_ORDERS = (1025, 262145)
LAUNCHES = 4
ROW, MAX_ROWS, STATE_WORDS = 32, 256, 44  # kPartial, kAlignMaxBlocks, sizeof(AlignState) / 4 (csrc/registration.hip)
SUMS = 29  # words of a partial row that do not depend on how a correspondence was found: 28 sums and the inlier count


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_spd_covs(n, seed):
    """n covariances in the stored layout (16 floats: a 4x4 whose 3x3 block counts), B B^T + 1e-4 I with B ~ N(0, 0.05^2)"""
    B = np.random.RandomState(seed).normal(0.0, 0.05, size=(n, 3, 3))
    C3 = B @ B.transpose(0, 2, 1) + 1e-4 * np.eye(3)
    out = np.zeros((n, 4, 4), np.float32)
    out[:, :3, :3] = C3.astype(np.float32)
    out[:, :3, :3] = 0.5 * (out[:, :3, :3] + out[:, :3, :3].transpose(0, 2, 1))  # symmetric in float32 too
    return out.reshape(n, 16)


@pytest.fixture(scope="module")
def scene(sp):
    """test_gpu_source_tiles.py's scene: a small target with a known pose (config 4's density and twist), its covariances from
    20 neighbours, random SPD source covariances. The source's first 3000 points are the target's counterpart cloud; the sizes
    beyond that continue with uniform points of the target's box, moved by the same pose (every one has a nearest target)."""
    from sycl_points_amd.synthetic import Mt19937Cloud, gicp_pair

    R = 10.0 * (N_TARGET / 1e6) ** (1.0 / 3.0)
    src, tgt, T_gt = gicp_pair(N_TARGET, R, seed=2718)
    more = Mt19937Cloud(31415).uniform_points(N_MAX - N_TARGET, R)
    Tinv = np.linalg.inv(T_gt.astype(np.float64))
    more[:, :3] = (more[:, :3].astype(np.float64) @ Tinv[:3, :3].T + Tinv[:3, 3]).astype(np.float32)
    src = np.concatenate([src, more]).astype(np.float32)
    Tg = sp.PointCloudShared(dev(tgt))
    Tg.covs = sp.GridKNN.build(Tg.points, points_per_cell=6.0).self_knn(20, want_knn=False, want_covs=True)[1]
    grid = sp.GridKNN.build(Tg.points)
    prep = sp.PreparedTarget(grid, Tg.covs)
    ref_grid = sp.GridKNN.build(Tg.points, points_per_cell=4.0)  # the independent search's own structure
    scov = random_spd_covs(N_MAX, 5)
    T0 = T_gt.copy()
    T0[:3, 3] += np.float32(grid.cell_size()) * np.float32([0.6, -0.6, 0.5])  # |.| = 0.98 cells off the truth
    return dict(src=src, scov=scov, Tg=Tg, grid=grid, prep=prep, ref_grid=ref_grid, T_gt=T_gt, T0=T0)


def fill_tiles_nan(sp, psrc):
    L = sp._lib.lib()
    nf = L.sp_internal_source_tile_floats(psrc._h)
    buf = torch.full((nf,), float("nan"), dtype=torch.float32, device="cuda")
    sp.check(L.sp_internal_source_tiles_copy(psrc._h, sp._ptr(buf), nf, 1, sp._stream()))
    torch.cuda.synchronize()


def T16(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(-1).copy()  # column-major, as the device holds a pose


def step_launches(sp, sc, n, mode, reuse):
    """LAUNCHES launches of sp_gicp_align_step (one GPU, criteria 0) + the finish; what every launch left behind, as numpy."""
    L = sp._lib.lib()
    S = sp.PointCloudShared(dev(sc["src"][:n]), covs=dev(sc["scov"][:n]))
    reg = sp.Registration(sp.RegistrationParams(criteria_translation=0.0, criteria_rotation=0.0, max_iterations=LAUNCHES))
    if reuse is not None:
        reg._set_source_option("reuse", reuse)
    psrc, _ = reg._prepared_source(n)
    fill_tiles_nan(sp, psrc)
    T_dev = dev(T16(sc["T0"]))
    psrc.prepare(sc["prep"], S, T_dev, mode)
    ws, lin = reg._buffers(T_dev.device)
    wsf = ws.view(torch.float32)
    nlog = C.c_size_t(0)
    log_word = (L.sp_internal_align_searched_log(sp._ptr(ws), C.byref(nlog)) - ws.data_ptr()) // 4
    state_word = log_word - 2 * STATE_WORDS  # the two AlignState blocks lie right in front of the log (align_ws)
    fp = reg._factor_params(reg.params.robust_default_scale)
    gn = sp._lib.GnParams(reg.params.gn_lambda, 0.0, 0.0)
    nn_idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    nn_d2 = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    grid_rows = min((n + 1023) // 1024, MAX_ROWS)
    out = []
    for k in range(LAUNCHES):
        nn_idx.fill_(-7)
        nn_d2.fill_(float("nan"))
        sp.check(L.sp_gicp_align_step(sc["prep"]._h, psrc._h, sp._ptr(T_dev), C.byref(fp), C.byref(gn), k, 0, sp._ptr(nn_idx),
                                      sp._ptr(nn_d2), sp._ptr(lin), sp._ptr(ws), ws.numel(), sp._stream()))
        torch.cuda.synchronize()
        rows = wsf[(k & 1) * MAX_ROWS * ROW:(k & 1) * MAX_ROWS * ROW + grid_rows * ROW].cpu().numpy().reshape(grid_rows, ROW).copy()
        rec = dict(nn_idx=nn_idx.cpu().numpy().copy(), nn_d2=nn_d2.cpu().numpy().copy(), rows=rows)
        if k == 0:
            rec["pose"] = T_dev.clone()
        else:  # the launch's prologue finished iteration k - 1: its state, its system, and the pose this launch linearised at
            s0 = state_word + ((k - 1) & 1) * STATE_WORDS
            rec["state"] = wsf[s0:s0 + STATE_WORDS].cpu().numpy().copy()
            rec["lin"] = lin.cpu().numpy().copy()
            rec["pose"] = wsf[s0:s0 + 16].clone()
        out.append(rec)
    delta = torch.zeros(8, dtype=torch.float32, device="cuda")
    sp.check(L.sp_gicp_align_finish(psrc._h, sp._ptr(T_dev), C.byref(gn), LAUNCHES - 1, 0, sp._ptr(lin), sp._ptr(delta), None,
                                    sp._ptr(ws), ws.numel(), sp._stream()))
    torch.cuda.synchronize()
    final = dict(T=T_dev.cpu().numpy().copy(), lin=lin.cpu().numpy().copy(), delta=delta.cpu().numpy().copy())
    return S, out, final


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


CASES = [(n, "presorted") for n in NS] + [(n, True) for n in BOTH_ORDERS]


@pytest.mark.parametrize("n,mode", CASES, ids=[f"{n}-{'presorted' if m == 'presorted' else 'sort-by-cell'}" for n, m in CASES])
def test_every_launch_against_an_independent_search_and_against_no_reuse(sp, scene, n, mode):
    S, on, fin_on = step_launches(sp, scene, n, mode, None)  # the shipped reuse
    _, off, fin_off = step_launches(sp, scene, n, mode, 0)
    searched_on = []
    for k in range(LAUNCHES):
        a, b = on[k], off[k]
        # the independent search at the pose of this launch
        r1 = scene["ref_grid"].knn_search(S, 1, transT=a["pose"])
        r2 = scene["ref_grid"].knn_search(S, 2, transT=a["pose"])
        want = r1.indices.cpu().numpy().reshape(n)
        d12 = r2.distances.cpu().numpy().reshape(n, 2)
        assert (d12[:, 0] < d12[:, 1]).all(), "two targets at the same distance from a query: the clouds are not random"
        assert np.array_equal(r2.indices.cpu().numpy().reshape(n, 2)[:, 0], want)
        wrong = np.flatnonzero(a["nn_idx"] != want)
        print(f"n={n} launch {k}: {wrong.size} neighbours differ from the independent search"
              f", max |d2 - d2_ref| = {np.abs(a['nn_d2'] - d12[:, 0]).max():.3e}")
        assert wrong.size == 0, (k, wrong[:8], a["nn_idx"][wrong[:8]], want[wrong[:8]])  # (-7: a point was left out)
        assert np.array_equal(b["nn_idx"], want)
        # reuse on == reuse off, bit for bit
        assert np.array_equal(bits(a["nn_d2"]), bits(b["nn_d2"])), k
        assert np.array_equal(bits(a["rows"][:, :SUMS]), bits(b["rows"][:, :SUMS])), k
        # no NaN of an unused lane reached a sum (a row's last two words are not written)
        assert np.isfinite(a["rows"][:, :SUMS + 1]).all() and np.isfinite(a["nn_d2"]).all()
        assert int(a["rows"][:, 28].view(np.uint32).sum()) == n  # every point is an inlier of this scene: none left out, none twice
        assert b["rows"][:, 29].sum() == n and 0 <= a["rows"][:, 29].sum() <= n  # searched points: all | some
        searched_on.append(int(a["rows"][:, 29].sum()))
        if k > 0:
            assert np.array_equal(bits(a["state"][:42]), bits(b["state"][:42])), k  # pose, linearisation pose, delta, flags
            assert bits(b["state"])[42] == n and bits(a["state"])[42] == searched_on[k - 1]
            assert np.array_equal(bits(a["lin"]), bits(b["lin"])), k
            assert np.isfinite(a["state"][:40]).all() and np.isfinite(a["lin"][:44]).all()
    for x, y in zip(fin_on.values(), fin_off.values()):
        assert np.array_equal(bits(x), bits(y))
    print(f"n={n}: searched per launch with reuse on = {searched_on}")
    assert searched_on[0] == n  # the cache holds nothing yet
    if n >= 1024:  # launches 1-3 took both paths: rows that held (prefetched and used) and rows that did not (searched)
        assert 0 < sum(searched_on[1:]) < 3 * n, searched_on


def align_fused(sp, sc, n, p, reuse, mode, persistent):
    S = sp.PointCloudShared(dev(sc["src"][:n]), covs=dev(sc["scov"][:n]))
    reg = sp.Registration(p)
    if reuse is not None:
        reg._set_source_option("reuse", reuse)
    reg._set_source_option("persistent", persistent)
    psrc, _ = reg._prepared_source(n)
    fill_tiles_nan(sp, psrc)
    T_dev, lin, delta = reg.align_fused_loop(S, sc["prep"], sort_by_cell=mode)
    torch.cuda.synchronize()
    return (T_dev.cpu().numpy().copy(), lin.cpu().numpy().copy(), delta.cpu().numpy().copy(),
            reg._iters_dev.cpu().numpy().copy()), S


@pytest.mark.parametrize("criteria", [1e-3, 0.0], ids=["default-criteria", "criteria-0-six-iterations"])
@pytest.mark.parametrize("persistent", [1, 0], ids=["shipped-form", "a-launch-per-iteration"])
@pytest.mark.parametrize("n", BOTH_ORDERS)
def test_whole_alignment_bytes_of_no_reuse_repeatable_and_generic_parity(sp, scene, n, persistent, criteria):
    """default criteria with a launch per iteration: the launch whose prologue finds the step converged, and every launch
    after it, return with the first trip's loads outstanding"""
    p = sp.RegistrationParams(criteria_translation=criteria, criteria_rotation=criteria, max_iterations=20 if criteria > 0 else 6)
    on, S = align_fused(sp, scene, n, p, None, "presorted", persistent)
    again, _ = align_fused(sp, scene, n, p, None, "presorted", persistent)
    off, _ = align_fused(sp, scene, n, p, 0, "presorted", persistent)
    for a, b, c in zip(on, again, off):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
        assert np.isfinite(a.astype(np.float64)[:44]).all()
    iters = int(on[3][0])
    assert (iters < 20) if criteria > 0 else (iters == 6), iters
    lin = sp.Registration._read_lin(torch.from_numpy(on[1]))
    assert lin.inlier == n
    regg = sp.Registration(p)
    Tgen, _, _ = regg.align_device_loop(S, scene["Tg"], scene["grid"], iterations=iters)
    T = on[0].reshape(4, 4).T
    diff = np.abs(regg.T_from_device(Tgen) - T).max()
    print(f"n={n} criteria={criteria} persistent={persistent}: {iters} iterations, |T_fused - T_generic| = {diff:.3e}, "
          f"|T_fused - T_gt| = {np.abs(T - scene['T_gt']).max():.3e}")
    assert diff < 2e-6  # test_gpu_source_tiles.py's tolerance against the generic loop
