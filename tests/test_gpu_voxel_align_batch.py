"""Registration.align_voxel_map_batch / Registration::align_batch(source, map, guesses) over sp_vhm_align_batch
(csrc/voxel_registration_batch.hip): the alignment of one scan against a VoxelHashMap from many initial guesses in one launch, a
workgroup per guess.

Sizes: sources of 64 points (the 256-lane form, most lanes idle), 257 (the first size of the 512-lane form) and 513 (a second pass
with one live lane; 512 is the table's workgroup size for 1, 7 and 27 cells); batches of 1, 3 and 257 (more workgroups than
compute units).

  1. the first linearisation (GN, one iteration) against the float64 model of tests/f64_voxel_registration.py on its engineered
     scene and on its first 128 points: keys and inliers exact, H / b / error_raw within TOL_F64 per block; also after a rehash
  2. whole alignments against the sequential trace (tests/voxel_align_trace.py: the host stepper over sp_vhm_linearize /
     sp_vhm_error), by the rule of tests/test_gpu_optimize.py's check_against_oracle with the trace in the oracle's place
  3. frozen correspondences: keys and the block's H, b are those of a linearisation at T_lin
  4. a hypothesis's defined result bytes are the same in batches of 1, 3, 257 and in two runs; T_out may alias T_init
  5. a hopeless guess ends with no inlier, as the trace does, and changes nothing next to it
  6. the map is untouched: an sp_vhm_error on a linearisation made before the batch gives the same bits after it
  7. on a capturing stream, and with persistent launches switched off on another Registration's prepared source
  8. argument errors: code, message, result buffer untouched
  9. the C++ facade (tests/cpp/test_voxel_align_batch.cpp)

The two implementations differ only in the summation tree (one workgroup's LDS tree against 256-lane partial rows and a second
launch). `pytest -s` prints every figure before it is asserted. MEASURED below holds the figures of an MI355X run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f64_factors as f64
import f64_voxel_registration as vr
from test_gpu_lidar_odometry import build
from test_gpu_voxel_registration import (World, cloud, dev, export_of, planes_scene, pose_errors, registration, scene_map,
                                         with_covariances)
from voxel_align_trace import trace

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
TOL_F64 = 2e-4  # the project's float32-against-float64 bound (f64.distances, per block)
TOL = 2e-4      # check_against_oracle's margin
SIZES = (64, 257, 513)

MEASURED = """
First linearisation against float64 (worst block of H / half of b / error_raw), keys equal everywhere, inliers 110 / 219 / 235 of 288
and 45 / 97 / 106 of 128 with 1 / 7 / 27 cells:   GICP + NONE 1.5e-5 (b, 1 cell)   GICP + GEMAN_MCCLURE 4.3e-6
  POINT_TO_DISTRIBUTION 3.4e-6 (both losses)   after a rehash 4.9e-6
Whole alignments against the sequential trace, 108 (case, cells, n, hypothesis) combinations: pose <= 6.0e-8, logged errors <= 1.0e-5
up to the first decision inside the margin; sixteen combinations held to their first decision only, all from the ground truth.
  GN + POINT_TO_DISTRIBUTION + CAUCHY: 6 iterations from the start and the twists, 4 from the ground truth, every decision outside
  the margin.
Frozen correspondences: keys equal, H / b / error within 5.6e-7 of a linearisation at T_lin (0 with 64 and 257 points).
A hopeless guess: no inlier, iterations / converged / steps as the trace (LM: 0 iterations, converged; dog-leg: 24, not converged).
C++ facade against align_voxel_map_batch: the same bits in all four poses; yaw sweep: 5, 35 and 335 degrees end in the same optimum
with 513 inliers, 2.1e-3 m from the known motion.
"""

CASES = [
    dict(opt="LM", reg_type="GICP", loss="GEMAN_MCCLURE", scales=[1.0], cells=(1, 7, 27)),
    dict(opt="DOGLEG", reg_type="GICP", loss="NONE", scales=[1.0], cells=(1, 7)),
    dict(opt="GN", reg_type="POINT_TO_DISTRIBUTION", loss="CAUCHY", scales=[10.0], cells=(1, 7)),
    dict(opt="LM", reg_type="GICP", loss="GEMAN_MCCLURE", scales=[10.0, 5.0, 2.5], cells=(1, 7)),  # annealing
]
CASE_IDS = [f"{c['opt']}-{c['reg_type']}-{c['loss']}-{len(c['scales'])}" for c in CASES]
PAIRS = [(c, cells) for c in CASES for cells in c["cells"]]
PAIR_IDS = [f"{CASE_IDS[CASES.index(c)]}-{cells}cells" for c, cells in PAIRS]
# the scene's start (identity), two twists inside the basin, the ground truth
TWISTS = {"small": [0.01, -0.005, 0.02, 0.05, -0.04, 0.03], "large": [-0.02, 0.015, -0.01, -0.06, 0.05, 0.04]}
HYPOTHESES = ("identity", "small", "large", "gt")
# (case, cells, n, hypothesis) -> the number of decisions the trace leaves outside the margin, where that is fewer than two
# (asserted: the table cannot widen by itself); such a pair is held to those decisions only
# Starting AT the ground truth the first iteration still decides something (the noisy source's optimum is a little off), every
# later one compares two errors of a converged alignment: for any implementation, whatever the parameters.
FIRST_DECISION_ONLY = {(cid, cells, n, "gt"): 1 for cid, cells, sizes in (
    ("LM-GICP-GEMAN_MCCLURE-1", 1, (513,)), ("LM-GICP-GEMAN_MCCLURE-1", 7, (257, 513)), ("LM-GICP-GEMAN_MCCLURE-1", 27, (257, 513)),
    ("DOGLEG-GICP-NONE-1", 1, (64, 257, 513)), ("DOGLEG-GICP-NONE-1", 7, (64, 257, 513)),
    ("LM-GICP-GEMAN_MCCLURE-3", 1, (64, 257, 513)), ("LM-GICP-GEMAN_MCCLURE-3", 7, (257, 513))) for n in sizes}


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from sycl_points_amd import _lib

    _lib.build()
    import sycl_points_amd.api as api

    return api


def defined(block):
    """the bytes of an sp_align_result that its writer defines: everything in front of the log, and the log's entries"""
    from sycl_points_amd import _lib

    r = _lib.AlignResult.from_buffer_copy(block)
    assert r.pad[0] == 0x600DF00D and r.status == 0  # SP_ALIGN_RESULT_DONE
    return block[:_lib.AlignResult.log.offset + r.log_entries * C.sizeof(_lib.OptLogEntry)]


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.fixture(scope="module")
def world(sp):
    w = World(sp)
    bad, _ = vr.scene_report(w.scene, w.export)
    assert not bad, bad[:10]
    w.models = {}
    return w


def model(w, export, tag, npts, mode, factor, loss):
    """the float64 system of the scene's first npts source points at scene["T"], and the robust scale of the whole scene"""
    key = (tag, npts, mode, factor, loss)
    if key not in w.models:
        _, s = w.ref(mode, factor, loss)
        src, scov = w.scene["src"][:npts], w.scene["scov"][:npts]
        nn, d2, keys = vr.correspondences(export, src, w.scene["T"], mode)
        case = vr.case_for(export, src, scov, w.scene["T"], nn, d2)
        w.models[key] = (f64.system_fast(case, factor, loss, s), s, keys)
    return w.models[key]


def check_first_linearisation(w, m, export, tag, npts, mode, factor, loss):
    ref, s, keys = model(w, export, tag, npts, mode, factor, loss)
    source = cloud(w.sp, w.scene["src"][:npts], w.scene["scov"][:npts])
    reg = registration(w.sp, factor, loss, optimization_method="GN", max_iterations=1)
    res = reg.align_voxel_map_batch(source, w.prepared(factor, m), [w.scene["T"]], [s], mode, want_keys=True)[0]
    got_keys = res.keys.cpu().numpy().view(np.uint64)
    d = f64.distances(res.H, res.b, res.error_raw, ref)
    print(f"\n[voxel align batch] {tag} n {npts} cells {mode:2d} {factor:22s} {loss:14s} inlier {res.inlier:3d} / {ref['inlier']:3d}  "
          f"keys differing {(got_keys != keys).sum()}  " + "  ".join(f"{k} {v:.1e}" for k, v in d.items()), end="")
    assert np.array_equal(got_keys, keys)
    assert res.inlier == ref["inlier"] and ref["inlier"] >= 20
    assert max(d.values()) <= TOL_F64, d
    assert res.linearizations == 1 and res.trials == 0 and res.searched == npts and res.iterations == 0
    assert np.array_equal(res.T_lin, w.scene["T"])


@pytest.mark.parametrize("loss", ("NONE", "GEMAN_MCCLURE"))
@pytest.mark.parametrize("factor", ("GICP", "POINT_TO_DISTRIBUTION"))
@pytest.mark.parametrize("mode", (1, 7, 27))
def test_first_linearisation_matches_float64_model(world, mode, factor, loss):
    n = len(world.scene["src"])
    assert n == 288
    for npts in (n, 128):  # the 512-lane form, the 256-lane form
        check_first_linearisation(world, world.map, world.export, "scene", npts, mode, factor, loss)


def test_first_linearisation_after_a_rehash(world):
    w = world
    m = w.sp.VoxelHashMap(vr.VOXEL_SIZE)
    m.set_min_num_point(vr.MIN_NUM_POINT)
    m.set_rehash_threshold(1e-4)
    n = len(w.scene["tgt"])
    for lo, hi in ((0, n // 2), (n // 2, n)):
        m.add_point_cloud(cloud(w.sp, w.scene["tgt"][lo:hi], w.scene["tcov"][lo:hi]))
    assert m.info("capacity") == 60013
    exp = export_of(m)
    assert set(exp.row) == set(w.export.row)
    for npts in (288, 128):
        check_first_linearisation(w, m, exp, "grown", npts, 7, "GICP", "NONE")


# ------------------------------------------------------------------------------------------------ 2 - 7. the planes
@pytest.fixture(scope="module")
def planes(sp):
    from scipy.linalg import expm

    tgt, src, T_true = planes_scene()
    source = with_covariances(sp, src)
    # The map: ONE point per voxel, computed on the host (the mean of the scene's points in the cell and their sample covariance
    # + 0.02 I, cells with at least 5 points). A map accumulates with float atomics, whose order is not fixed: built from the
    # 20 100 points its last bits differ from run to run, and with them every decision that compares two errors of a converged
    # alignment. (The 0.02 I keeps the determinant above the 1e-6 below which point-to-distribution's inverse is zero.)
    p64 = tgt[:, :3].astype(np.float64)
    cells, inverse, counts = np.unique(np.floor(p64 / 0.5).astype(np.int64), axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    means, covs = [], []
    for c in np.nonzero(counts >= 5)[0]:
        q = p64[inverse == c]
        means.append(q.mean(axis=0))
        covs.append(np.cov(q.T) + 0.02 * np.eye(3))
    mp = np.ones((len(means), 4), np.float32)
    mp[:, :3] = np.array(means)
    assert len(means) > 500 and (np.floor(mp[:, :3].astype(np.float64) / 0.5) == cells[counts >= 5]).all()
    m = sp.VoxelHashMap(0.5)
    m.add_point_cloud(cloud(sp, mp, f64.cov16(np.array(covs).astype(np.float32))))
    S = {n: sp.PointCloudShared(source.points[:n].contiguous(), covs=source.covs[:n].contiguous()) for n in SIZES}
    T = {k: expm(f64.twist_matrix(np.array(v))).astype(np.float32) for k, v in TWISTS.items()}
    T["identity"] = np.eye(4, dtype=np.float32)
    T["gt"] = T_true.astype(np.float32)
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 1000.0
    T["far"] = far
    return {"map": m, "S": S, "T": T, "T_true": T_true, "traces": {}}


def reg_of(sp, case):
    return sp.Registration(sp.RegistrationParams(reg_type=case["reg_type"], robust_type=case["loss"], robust_default_scale=case["scales"][0],
                                                 optimization_method=case["opt"], max_correspondence_distance=1.0,
                                                 max_iterations=25 if len(case["scales"]) == 1 else 10))


def trace_of(sp, planes, case, cells, n, name):
    key = (CASE_IDS[CASES.index(case)], cells, n, name)
    if key not in planes["traces"]:
        planes["traces"][key] = trace(sp, reg_of(sp, case), planes["S"][n], planes["map"], planes["T"][name], case["scales"], cells)
    return planes["traces"][key]


def check_against_trace(res, ref, steps, tag, levels, first_only):
    """check_against_oracle of tests/test_gpu_optimize.py, the trace in the oracle's place"""
    dT = np.abs(res.T - ref.T).max()
    got = [(e["trials"], e["accepted"]) for e in res.log]
    want = [(s["trials"], s["accepted"]) for s in steps]
    decided = next((i for i, s in enumerate(steps) if s["margin"] < TOL), len(want))
    worst_e = max([abs(e["error"] - s["error"]) / abs(s["error"]) for e, s in zip(res.log[:decided], steps[:decided]) if s["error"]] + [0.0])
    print(f"\n[voxel align batch] {tag}: pose {dT:.2e}, {len(got)} / {len(want)} iterations, {decided} decided, worst error {worst_e:.1e}, "
          f"inlier {res.inlier} / {ref.inlier}, lin {res.linearizations} trials {res.trials} searched {res.searched}", end="")
    if first_only is not None:
        assert decided == first_only < min(2, len(want))
    else:
        assert decided >= min(2, len(want)), "a hypothesis whose FIRST decisions are inside rounding checks nothing: pick another"
    assert got[:decided] == want[:decided], (tag, got, want, decided)
    for e, s in zip(res.log[:decided], steps[:decided]):
        assert abs(e["damping"] - s["damping"]) <= 1e-6 * abs(s["damping"]), (tag, e, s)
        assert abs(e["error"] - s["error"]) <= 2e-4 * abs(s["error"]), (tag, e, s)
    if decided == len(want):
        assert got == want
        assert res.converged == ref.converged and res.iterations == ref.iterations, tag
        assert res.inlier == ref.inlier
        assert res.linearizations == ref.linearizations == len(want) and res.trials == ref.trials == sum(t for t, _ in want)
    assert dT < 1e-5, (tag, dT)  # whatever the decisions: the rule's first line
    assert max(e["level"] for e in res.log) == levels - 1


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_every_hypothesis_matches_the_sequential_trace(sp, planes, pair):
    case, cells = pair
    cid = CASE_IDS[CASES.index(case)]
    failed = []  # (every hypothesis is looked at before the test fails: the figures of all of them are printed)
    for n in SIZES:
        results = reg_of(sp, case).align_voxel_map_batch(planes["S"][n], planes["map"], [planes["T"][k] for k in HYPOTHESES],
                                                         case["scales"], cells)
        assert len(results) == len(HYPOTHESES)
        for name, res in zip(HYPOTHESES, results):
            ref, steps = trace_of(sp, planes, case, cells, n, name)
            assert res.searched == n * res.linearizations  # every linearisation looks every point up
            try:
                check_against_trace(res, ref, steps, f"{cid} {cells} cells n={n} {name}", len(case["scales"]),
                                    FIRST_DECISION_ONLY.get((cid, cells, n, name)))
            except AssertionError as e:
                failed.append((n, name, str(e)[:300]))
    assert not failed, failed


@pytest.mark.parametrize("n", SIZES)
def test_frozen_correspondences(sp, planes, n):
    case, cells = CASES[0], 7
    reg = reg_of(sp, case)
    S, m = planes["S"][n], planes["map"]
    results = reg.align_voxel_map_batch(S, m, [planes["T"][k] for k in HYPOTHESES], case["scales"], cells, want_keys=True)
    for name, res in zip(HYPOTHESES, results):
        lin = reg.linearize_voxel_map(S, m, res.T_lin, case["scales"][-1], cells, want_keys=True)
        d = f64.distances(res.H, res.b, res.error_raw, {"H": lin["H"].astype(np.float64), "b": lin["b"].astype(np.float64), "error": lin["error"]})
        print(f"\n[voxel align batch] frozen n={n} {name}: keys differing {int((res.keys != lin['keys']).sum())}  "
              + "  ".join(f"{k} {v:.1e}" for k, v in d.items()), end="")
        assert torch.equal(res.keys, lin["keys"])
        assert max(d.values()) <= 2e-4, d


@pytest.mark.parametrize("n", SIZES)
def test_a_result_does_not_depend_on_the_batch_around_it(sp, planes, n):
    case, cells = CASES[3], 7
    reg = reg_of(sp, case)
    S, m, T = planes["S"][n], planes["map"], planes["T"]
    run = lambda guesses, **kw: reg._align_voxel_map_batch(S, m, guesses, case["scales"], cells, **kw)  # noqa: E731
    alone = run([T["large"]])[0]
    again = run([T["large"]])[0]
    three = run([T["identity"], T["large"], T["small"]])
    crowd = run([T["small"]] * 100 + [T["large"]] + [T["small"]] * 156)  # more workgroups than compute units
    apart = run([T["identity"], T["large"], T["small"]], T_out=torch.zeros(48, dtype=torch.float32, device="cuda"))
    assert len(crowd) == 257 and len(alone.log) >= 3
    want = defined(alone.block)
    assert defined(again.block) == want and defined(three[1].block) == want and defined(crowd[100].block) == want
    assert {defined(r.block) for i, r in enumerate(crowd) if i != 100} == {defined(three[2].block)}
    assert [defined(r.block) for r in apart] == [defined(r.block) for r in three]  # T_out aliasing T_init or not: the same


@pytest.mark.parametrize("case", CASES[:2], ids=CASE_IDS[:2])
def test_a_hopeless_guess_beside_good_ones(sp, planes, case):
    n, cells = 513, 1
    reg = reg_of(sp, case)
    S, m, T = planes["S"][n], planes["map"], planes["T"]
    clean = reg.align_voxel_map_batch(S, m, [T["small"], T["large"]], case["scales"], cells)
    mixed = reg.align_voxel_map_batch(S, m, [T["small"], T["far"], T["large"]], case["scales"], cells)
    far = mixed[1]
    ref, steps = trace_of(sp, planes, case, cells, n, "far")
    print(f"\n[voxel align batch] far: inlier {far.inlier}, iterations {far.iterations}, converged {far.converged}; trace "
          f"inlier {ref.inlier}, iterations {ref.iterations}, converged {ref.converged}", end="")
    assert far.inlier == 0 and ref.inlier == 0
    assert (far.iterations, far.converged, far.linearizations, far.trials) == (ref.iterations, ref.converged, ref.linearizations, ref.trials)
    assert defined(mixed[0].block) == defined(clean[0].block) and defined(mixed[2].block) == defined(clean[1].block)
    assert reg.best_of(mixed) in (0, 2) and reg.best_of([far]) == 1


def test_the_map_is_untouched(sp, planes):
    case, cells, n = CASES[0], 7, 257
    S, m, T = planes["S"][n], planes["map"], planes["T"]
    reg, other = reg_of(sp, case), reg_of(sp, case)
    if not m.registration_ready("GICP"):
        m.prepare_registration("GICP")
    lin = reg.linearize_voxel_map(S, m, T["small"], case["scales"][0], cells)
    before = reg.error_voxel_map(S, m, T["large"], case["scales"][0])
    for who in (other, reg):  # another object's buffers, then the very object whose workspace holds the frozen slots
        who.align_voxel_map_batch(S, m, [T["identity"], T["far"], T["gt"]], case["scales"], cells)
        assert m.registration_ready("GICP") and not m.registration_ready("POINT_TO_DISTRIBUTION")
        after = reg.error_voxel_map(S, m, T["large"], case["scales"][0])  # (would fail had the generation or the bookkeeping moved)
        assert after == before and after[1] == lin["inlier"]


def test_on_a_capturing_stream_and_without_persistent_launches(sp, planes):
    from sycl_points_amd import _lib

    case, cells, n = CASES[0], 7, 513
    S, m, T = planes["S"][n], planes["map"], planes["T"]
    guesses = [T["small"], T["large"], T["identity"]]
    reg = reg_of(sp, case)
    want = reg.align_voxel_map_batch(S, m, guesses, case["scales"], cells)
    L = _lib.lib()
    # persistent launches switched off on a prepared source of the same Registration: the batch needs none
    psrc, _ = reg._prepared_source(n)
    sp.check(L.sp_gicp_source_set_persistent(psrc._h, 0))
    again = reg.align_voxel_map_batch(S, m, guesses, case["scales"], cells)
    assert [defined(r.block) for r in again] == [defined(r.block) for r in want]
    # captured: both launches of the call, replayed with the poses put back
    T_dev, res_dev, _, ws = reg._batch_bufs
    rsz, B = C.sizeof(_lib.AlignResult), len(guesses)
    poses = torch.from_numpy(np.stack([np.ascontiguousarray(g.T).reshape(-1) for g in guesses]).reshape(-1).copy()).cuda()
    fp, op, sc = reg._factor_params(case["scales"][0]), reg.opt_params(), (C.c_float * 1)(case["scales"][0])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = L.sp_vhm_align_batch(m._h, sp._ptr(S.points), sp._ptr(S.covs), n, sp._ptr(T_dev), sp._ptr(T_dev), B, C.byref(fp), C.byref(op),
                                  sc, 1, cells, sp._ptr(res_dev), None, sp._ptr(ws), ws.numel(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.sp_last_error()
    for _ in range(2):
        T_dev[:16 * B].copy_(poses)
        res_dev.zero_()
        g.replay()
        torch.cuda.synchronize()
        raw = res_dev[:rsz * B].cpu().numpy().tobytes()
        assert [defined(raw[rsz * b:rsz * (b + 1)]) for b in range(B)] == [defined(r.block) for r in want]
        assert np.array_equal(T_dev[:16].cpu().numpy().reshape(4, 4).T, want[0].T)


# ------------------------------------------------------------------------------------------------ 8. errors
def test_argument_errors(sp, world):
    from sycl_points_amd import _lib

    w = world
    S, T = w.source, w.scene["T"]
    n = S.size()
    rsz = C.sizeof(_lib.AlignResult)

    def refused(code, text, reg, source, m, guesses, **kw):
        results = torch.full((rsz * 4,), 7, dtype=torch.uint8, device="cuda")
        with pytest.raises(sp.SpError) as e:
            reg._align_voxel_map_batch(source, m, guesses, prepare=False, results=results, **kw)
        print(f"\n[voxel align batch] refused ({e.value.code}): {e.value}", end="")
        assert e.value.code == code and text in str(e.value), (code, text, str(e.value))
        torch.cuda.synchronize()
        assert bool((results == 7).all()), "a refused call wrote to its results"

    gicp, p2d = registration(sp, "GICP"), registration(sp, "POINT_TO_DISTRIBUTION")
    m = scene_map(sp, w.scene)
    not_ready = "call sp_vhm_prepare_registration"
    refused(1, not_ready, gicp, S, m, [T])  # before prepare
    m.prepare_registration("GICP")
    assert len(gicp._align_voxel_map_batch(S, m, [T, T], prepare=False)) == 2
    refused(1, not_ready, p2d, S, m, [T])  # rows of the other factor
    refused(1, "neighbor_voxels must be 1, 7 or 27", gicp, S, m, [T], neighbor_voxels=5)
    refused(1, "rotation constraint", registration(sp, "GICP", rotation_constraint_enable=True), S, m, [T])
    refused(1, "reg_type must be GICP or POINT_TO_DISTRIBUTION", registration(sp, "POINT_TO_PLANE"), S, m, [T])
    need = _lib.lib().sp_vhm_align_batch_workspace_bytes(n, 2)
    refused(1, "workspace too small", gicp, S, m, [T, T], workspace_bytes=need - 1)
    refused(1, "batch must be in 1..SP_ALIGN_BATCH_MAX", gicp, S, m, [])
    big = cloud(sp, np.tile(w.scene["src"], (57, 1))[:16385], np.tile(w.scene["scov"], (57, 1))[:16385])
    assert big.size() == 16385
    refused(1, "SP_VHM_ALIGN_BATCH_MAX_POINTS", registration(sp, "GICP"), big, m, [T])
    refused(2, "Covariance matrices of source and target must be pre-computed", gicp, cloud(sp, w.scene["src"]), m, [T])
    refused(1, "max_iterations must be in 1..65535", registration(sp, "GICP", max_iterations=0), S, m, [T])
    m.add_point_cloud(cloud(sp, w.scene["tgt"][:5], w.scene["tcov"][:5]))  # stale rows
    refused(1, not_ready, gicp, S, m, [T])
    assert len(gicp.align_voxel_map_batch(S, m, [T])) == 1  # (refreshed by the call itself unless told not to)
    bare = sp.VoxelHashMap(vr.VOXEL_SIZE)
    bare.add_point_cloud(cloud(sp, w.scene["tgt"]))
    refused(1, "no covariances", gicp, S, bare, [T])


# ------------------------------------------------------------------------------------------------ 9. the C++ facade
def test_cpp_facade(sp, planes, tmp_path):
    """Registration::align_batch(source, map, guesses) against align_voxel_map_batch, bit for bit, on maps built from one point per
    voxel (the export of the planes scene's map: see test_gpu_voxel_registration.test_cpp_facade); the fallback to align() per guess
    with NL-Reg on; best_of over a 12-step yaw sweep."""
    exe = build(os.path.join(CPP, "test_voxel_align_batch.cpp"), os.path.join(CPP, "test_voxel_align_batch"))
    means = planes["map"].downsampling(distance=1e7)
    tp, tc = means.points.cpu().numpy(), means.covs.cpu().numpy()
    S = planes["S"][513]
    spn, sc = S.points.cpu().numpy(), S.covs.cpu().numpy()
    guesses = [planes["T"][k] for k in HYPOTHESES]
    path = str(tmp_path / "planes.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(tp), len(spn), len(guesses)], np.int32).tobytes())
        for a in (tp, tc, spn, sc):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        for g in guesses + [planes["T_true"].astype(np.float32)]:
            f.write(np.ascontiguousarray(np.asarray(g, np.float32).T).tobytes())  # column-major
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-4000:]
    for name in ("batch_on_the_device", "sequential_fallback", "yaw_sweep"):
        assert f"[  OK  ] {name}" in r.stdout, name
    theirs, scalars = {}, {}
    for line in r.stdout.splitlines():
        if line.startswith("T "):
            name, *words = line[2:].split()
            theirs[name] = np.array([int(x, 16) for x in words], np.uint32).view(np.float32).reshape(4, 4).T
        elif line.startswith("R "):
            name, it, conv, inl, err = line[2:].split()
            scalars[name] = (int(it), bool(int(conv)), int(inl), int(err, 16))
    m = sp.VoxelHashMap(0.5)
    m.add_point_cloud(cloud(sp, tp, tc))
    reg = sp.Registration(sp.RegistrationParams(reg_type="GICP", optimization_method="LM", max_correspondence_distance=1.0,
                                                max_iterations=25))
    mine = reg.align_voxel_map_batch(S, m, guesses, neighbor_voxels=7)
    assert set(theirs) == {f"batch{i}" for i in range(len(guesses))}
    for i, res in enumerate(mine):
        d = np.abs(theirs[f"batch{i}"] - res.T).max()
        print(f"[voxel align batch] C++ against Python, guess {i}: max |dT| = {d:.3g}; against T_true {pose_errors(res.T, planes['T_true'])}")
        assert np.array_equal(theirs[f"batch{i}"].view(np.uint32), np.asarray(res.T, np.float32).view(np.uint32)), i
        mine_scalars = (res.iterations, res.converged, res.inlier, int(np.float32(res.error).view(np.uint32)))
        assert scalars[f"batch{i}"] == mine_scalars, (i, scalars[f"batch{i}"], mine_scalars)
