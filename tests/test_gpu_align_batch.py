"""Registration.align_batch (sp_gicp_align_batch, csrc/registration_batch.hip): the alignment of ONE prepared source against ONE
prepared target from many initial guesses in one launch, a workgroup per guess. Clouds: tests/test_gpu_optimize.py's smallest
pair, gicp_pair(900) at density 8, plus a source of 1025 points (two passes of 1024 lanes, one live lane in the second) and one
of 64 points (the 256-lane form, most lanes idle) against the same target.

  1. every hypothesis against the oracle's align() from the same guess, by check_against_oracle of tests/test_gpu_optimize.py
     (pose 1e-5; decisions, damping and error up to the first decision whose oracle margin is below 2e-4)
  2. hypotheses with no decision inside that margin: the single launch (align_optimize) from the same guess gives the same
     iterations / converged / inlier and a pose within 2e-6
  3. a hypothesis's result block does not depend on the batch around it — bit for bit, log included — in batches of 1, 3, 257
  4. a hopeless hypothesis (1000 m away) ends like align_optimize from it, with no inlier, and changes nothing next to it
  5. the prepared source's own correspondence cache is untouched
  6. available with persistent launches switched off and on a capturing stream
  7. argument errors
  8. the C++ facade (tests/cpp/test_align_batch.cpp)

THE HYPOTHESES were chosen with the oracle (CPU) so that their first two decisions lie outside the 2e-4 margin: identity, the
existing test's twist, a larger one inside the basin, and the ground truth. Starting AT the ground truth the first iteration still
decides something (the noisy source's optimum is 8e-4 away), every later one compares two errors of a converged alignment: with
dog-leg and with the three annealing levels the oracle's second decision from there has a margin of 1.8e-6 / 4.4e-7 — for any
implementation, whatever the parameters (each level is a fresh alignment from the optimum). Those two (case, ground truth) pairs
are listed in FIRST_DECISION_ONLY with the number of decisions the oracle leaves outside the margin (asserted: the table cannot
widen by itself); they are held to every decision up to that point, and to the oracle's pose: to 1e-5 when the whole path is the
oracle's, to the convergence criterion when it parts at the decision inside rounding (see there). All other pairs assert the two
decisions and the 1e-5.

Measured on an MI355X (`pytest -s` prints every figure before it is asserted): pose against the oracle
5.6e-9 .. 6.9e-8 over all pairs whose path is the oracle's, against the single launch 9.3e-10 .. 6.4e-8 with the same
iterations / converged / inlier everywhere; dog-leg from the ground truth parts from the oracle at its second decision (accepts
a step the oracle rejects, stops after 2 iterations where the oracle runs 25) and ends 1.9e-5 from it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_lidar_odometry import build
from test_gpu_optimize import check_against_oracle, dev, oracle_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp")

CASES = [
    dict(opt="LM", reg_type="GICP", loss="GEMAN_MCCLURE", scale=0.5, levels=1),
    dict(opt="DOGLEG", reg_type="GICP", loss="NONE", scale=10.0, levels=1),
    dict(opt="GN", reg_type="POINT_TO_DISTRIBUTION", loss="CAUCHY", scale=0.3, levels=1),
    dict(opt="LM", reg_type="GICP", loss="GEMAN_MCCLURE", scale=10.0, levels=3),  # annealing 10 / 5 / 2.5
]
CASE_IDS = [f"{c['opt']}-{c['reg_type']}-{c['loss']}-{c['levels']}" for c in CASES]
TWISTS = {"identity": [0.0] * 6, "small": [0.01, -0.005, 0.02, 0.05, -0.04, 0.03], "large": [-0.03, 0.04, -0.02, -0.1, 0.12, 0.08],
          "large_b": [0.04, -0.03, 0.05, 0.15, -0.1, 0.12]}
# hypotheses per source: the issue's four on the 900-point pair; on the two extra sources the ones whose first two decisions
# the oracle puts outside the margin in all four cases
# (dog-leg from "large" on the 1025-point source, and from "large_b" on the 900-point one, runs all 25 iterations without
# converging in the oracle: a path that may part after a decision inside rounding and not meet again)
HYPOTHESES = {900: ("identity", "small", "gt", "large"), 1025: ("small", "large_b"), 64: ("small", "large_b")}
FIRST_DECISION_ONLY = {("DOGLEG-GICP-NONE-1", 900, "gt"): 1, ("LM-GICP-GEMAN_MCCLURE-3", 900, "gt"): 1}
TOL = 2e-4  # check_against_oracle's margin


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from sycl_points_amd import _lib

    _lib.build()
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def world(sp, orc):
    """clouds, covariances, poses; device clouds; prepared targets per factor; a cache of oracle alignments"""
    from sycl_points_amd.synthetic import gicp_pair

    r = 10.0 * (900 * 8.0 / 1e6) ** (1.0 / 3.0)
    src, tgt, T_gt = gicp_pair(900, r, 1234)
    src2, tgt2, _ = gicp_pair(1025, r, 1234)
    assert np.array_equal(tgt2[:900], tgt)  # (the same stream: the longer source continues the shorter one)
    cov = lambda p: orc.cov_estimate(p, orc.kdtree_knn(orc.kdtree_build(p), p, 20)[0])  # noqa: E731
    scov, tcov, scov2 = cov(src), cov(tgt), cov(src2)
    w = dict(tgt=tgt, tcov=tcov, T_gt=T_gt, host={900: (src, scov), 1025: (src2, scov2), 64: (src[:64].copy(), scov[:64].copy())})
    w["S"] = {n: sp.PointCloudShared(dev(p), covs=dev(c)) for n, (p, c) in w["host"].items()}
    grid = sp.GridKNN.build(dev(tgt))
    w["prep"] = {rt: sp.PreparedTarget(grid, dev(tcov), reg_type=rt) for rt in ("GICP", "POINT_TO_DISTRIBUTION")}
    w["T"] = {k: orc.se3_exp(v) for k, v in TWISTS.items()}
    w["T"]["gt"] = T_gt
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 1000.0
    w["T"]["far"] = far
    w["refs"] = {}
    return w


def scales_of(orc, case):
    if case["levels"] == 1:
        return [case["scale"]]
    s = [float(v) for v in orc.robust_annealing_scales(case["loss"], True, 10.0, 10.0, 2.5, 3)]
    assert len(s) == 3 and abs(s[1] - 5.0) < 1e-5 and abs(s[2] - 2.5) < 1e-5
    return s


def iterations_of(case):
    return 25 if case["levels"] == 1 else 10


def oracle_ref(orc, world, case, n, name):
    key = (CASE_IDS[CASES.index(case)], n, name)
    if key not in world["refs"]:
        kw = dict(max_iterations=iterations_of(case))
        if case["levels"] == 3:
            kw.update(auto_scale=1, auto_scaling_iter=3, init_scale=10.0, min_scale=2.5)
        p, c = world["host"][n]
        world["refs"][key] = orc.registration_align(oracle_params(case, **kw), p, c, world["tgt"], world["tcov"],
                                                    init_T=world["T"][name], steps=True)
    return world["refs"][key]


def registration(sp, case):
    return sp.Registration(sp.RegistrationParams(reg_type=case["reg_type"], robust_type=case["loss"], robust_default_scale=case["scale"],
                                                 optimization_method=case["opt"], max_iterations=iterations_of(case)))


def defined(block):
    """the bytes of an sp_align_result that its writer defines: everything in front of the log, and the log's entries"""
    from sycl_points_amd import _lib

    r = _lib.AlignResult.from_buffer_copy(block)
    return block[:_lib.AlignResult.log.offset + r.log_entries * C.sizeof(_lib.OptLogEntry)]


def same_result(a, b):
    return (np.array_equal(a.T, b.T) and np.array_equal(a.T_lin, b.T_lin) and np.array_equal(a.H, b.H) and np.array_equal(a.b, b.b)
            and (a.error, a.error_raw, a.inlier, a.iterations, a.converged) == (b.error, b.error_raw, b.inlier, b.iterations, b.converged)
            and (a.linearizations, a.trials, a.searched, a.damping) == (b.linearizations, b.trials, b.searched, b.damping) and a.log == b.log)


@pytest.mark.parametrize("n", [900, 1025, 64])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_hypothesis_matches_the_oracle_and_the_single_launch(sp, orc, world, case, n):
    cid = CASE_IDS[CASES.index(case)]
    names = HYPOTHESES[n]
    S, prep, scales = world["S"][n], world["prep"][case["reg_type"]], scales_of(orc, case)
    reg = registration(sp, case)
    results = reg.align_batch(S, prep, [world["T"][k] for k in names], scales)
    assert len(results) == len(names)
    for name, res in zip(names, results):
        ref = oracle_ref(orc, world, case, n, name)
        want = len(ref["steps"])
        decided = next((i for i, s in enumerate(ref["steps"]) if s["margin"] < TOL), want)
        print(f"{cid} n={n} {name}: pose {np.abs(res.T - ref['T']).max():.2e}, {len(res.log)} / {want} iterations, {decided} decided, "
              f"inlier {res.inlier} / {ref['inlier']}, searched {res.searched}")
        assert res.searched >= n and res.linearizations >= 1  # (the first linearisation searches every point)
        if (cid, n, name) in FIRST_DECISION_ONLY:
            assert decided == FIRST_DECISION_ONLY[(cid, n, name)] < min(2, want)
            for e, s in zip(res.log[:decided], ref["steps"][:decided]):
                assert (e["trials"], e["accepted"]) == (s["trials"], s["accepted"])
                assert abs(e["damping"] - s["damping"]) <= 1e-6 * abs(s["damping"]) and abs(e["error"] - s["error"]) <= 2e-4 * abs(s["error"])
            # the pose: the oracle's to 1e-5 when the whole path is the oracle's. When the paths part at the decision inside rounding
            # (measured, dog-leg: the oracle rejects its second trial and 23 more and stays where its first step took it; the kernel
            # accepts the second, a step below the convergence criteria, and stops: 1.9e-5 apart) both have already taken the one
            # step that was decided outside rounding, and what follows are steps from the optimum of a converged alignment: every
            # such step that is taken ends the level (is_converged: below criteria = 1e-3), so the two ends are within one
            # criterion of each other per level
            same_path = [(e["trials"], e["accepted"]) for e in res.log] == [(s["trials"], s["accepted"]) for s in ref["steps"]]
            assert np.abs(res.T - ref["T"]).max() < (1e-5 if same_path else 1e-3 * case["levels"]), same_path
            continue
        assert decided >= min(2, want), "chosen with the oracle: the first two decisions are outside the margin"
        check_against_oracle(res, ref, case, levels=case["levels"])
        if decided == want:  # no decision inside rounding: the single launch must walk the same path
            single = registration(sp, case).align_optimize(S, prep, world["T"][name], scales)
            assert single is not None
            d = np.abs(single.T - res.T).max()
            print(f"    single launch: pose {d:.2e}, iterations {single.iterations}, inlier {single.inlier}")
            assert (single.iterations, single.converged, single.inlier) == (res.iterations, res.converged, res.inlier)
            assert d < 2e-6


@pytest.mark.parametrize("n", [900, 64])
def test_a_result_does_not_depend_on_the_batch_around_it(sp, orc, world, n):
    case = CASES[3]
    S, prep, scales = world["S"][n], world["prep"]["GICP"], scales_of(orc, case)
    T = world["T"]
    reg = registration(sp, case)
    # (one preparation for all batches: the pose a source is prepared at decides which lane handles which point, hence how the
    # sums are grouped — align_batch prepares at its first guess unless told not to)
    alone = reg.align_batch(S, prep, [T["large"]], scales)[0]
    three = reg.align_batch(S, prep, [T["identity"], T["large"], T["small"]], scales, prepare=False)
    moved = reg.align_batch(S, prep, [T["large"], T["small"], T["identity"]], scales, prepare=False)
    crowd = reg.align_batch(S, prep, [T["small"]] * 100 + [T["large"]] + [T["small"]] * 156, scales, prepare=False)  # more workgroups than compute units
    assert len(crowd) == 257 and len(alone.log) >= 3
    want = defined(alone.block)
    assert defined(three[1].block) == want and defined(moved[0].block) == want and defined(crowd[100].block) == want
    assert defined(three[2].block) == defined(moved[1].block) and defined(three[0].block) == defined(moved[2].block)
    copies = {defined(r.block) for i, r in enumerate(crowd) if i != 100}
    assert copies == {defined(three[2].block)}  # 256 copies of one guess: one block


@pytest.mark.parametrize("case", CASES[:2], ids=CASE_IDS[:2])
def test_a_hopeless_hypothesis_beside_good_ones(sp, orc, world, case):
    S, prep, scales = world["S"][900], world["prep"][case["reg_type"]], scales_of(orc, case)
    T = world["T"]
    reg = registration(sp, case)
    clean = reg.align_batch(S, prep, [T["small"], T["large"]], scales)
    mixed = reg.align_batch(S, prep, [T["small"], T["far"], T["large"]], scales, prepare=False)
    far = mixed[1]
    single = registration(sp, case).align_optimize(S, prep, T["far"], scales)
    assert single is not None
    print(f"far: inlier {far.inlier}, iterations {far.iterations}, converged {far.converged}, searched {far.searched}; single launch "
          f"iterations {single.iterations}, converged {single.converged}")
    assert far.inlier == 0 and _status(far) == 0
    assert (far.iterations, far.converged) == (single.iterations, single.converged) and single.inlier == 0
    assert defined(mixed[0].block) == defined(clean[0].block) and defined(mixed[2].block) == defined(clean[1].block)
    assert reg.best_of(mixed) in (0, 2)
    assert reg.best_of([far]) == 1 and reg.best_of([far, far]) == 2  # (no block qualifies)


def _status(res):
    from sycl_points_amd import _lib

    r = _lib.AlignResult.from_buffer_copy(res.block)
    assert r.pad[0] == 0x600DF00D  # SP_ALIGN_RESULT_DONE
    return r.status


def test_the_source_is_untouched(sp, orc, world):
    case = CASES[0]
    S, prep, T = world["S"][900], world["prep"]["GICP"], world["T"]
    out = []
    for with_batch in (False, True):
        reg = registration(sp, case)
        first = reg.align_optimize(S, prep, T["small"], [case["scale"]], prepare=True)
        if with_batch:
            reg.align_batch(S, prep, [T["identity"], T["large"], T["far"]], [case["scale"]], prepare=False)
        second = reg.align_optimize(S, prep, T["small"], [case["scale"]], prepare=False)
        assert first is not None and second is not None
        out.append((first, second))
    assert same_result(out[0][0], out[1][0])
    assert same_result(out[0][1], out[1][1]), (out[0][1].searched, out[1][1].searched)
    assert out[0][1].searched < out[0][0].searched  # (the second alignment did reuse the source's own rows)


def test_available_without_persistent_launches_and_on_a_capturing_stream(sp, orc, world):
    from sycl_points_amd import _lib

    case = CASES[0]
    S, prep, T = world["S"][900], world["prep"]["GICP"], world["T"]
    guesses = [T["small"], T["large"], T["identity"]]
    reg = registration(sp, case)
    want = reg.align_batch(S, prep, guesses, [case["scale"]])
    L = _lib.lib()
    sp.check(L.sp_gicp_source_set_persistent(reg._psrc._h, 0))
    assert reg.align_optimize(S, prep, T["small"], [case["scale"]]) is None  # the single launch is not available ...
    again = reg.align_batch(S, prep, guesses, [case["scale"]])  # ... the batch is
    assert [defined(r.block) for r in again] == [defined(r.block) for r in want]
    # captured: the call itself (one kernel), replayed with the poses put back
    T_dev, res_dev, _, ws = reg._batch_bufs
    rsz, B = C.sizeof(_lib.AlignResult), len(guesses)
    poses = torch.from_numpy(np.stack([np.ascontiguousarray(g.T).reshape(-1) for g in guesses]).reshape(-1).copy()).cuda()
    fp, op, sc = reg._factor_params(case["scale"]), reg.opt_params(), (C.c_float * 1)(case["scale"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = L.sp_gicp_align_batch(prep._h, reg._psrc._h, sp._ptr(T_dev), sp._ptr(T_dev), B, C.byref(fp), C.byref(op), sc, 1,
                                   sp._ptr(res_dev), sp._ptr(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.sp_last_error()
    for _ in range(2):
        T_dev[:16 * B].copy_(poses)
        res_dev.zero_()
        g.replay()
        torch.cuda.synchronize()
        raw = res_dev[:rsz * B].cpu().numpy().tobytes()
        assert [defined(raw[rsz * b:rsz * (b + 1)]) for b in range(B)] == [defined(r.block) for r in want]
        assert np.array_equal(T_dev[:16].cpu().numpy().reshape(4, 4).T, want[0].T)


def test_argument_errors(sp, orc, world):
    from sycl_points_amd import _lib

    case = CASES[0]
    S, prep, T = world["S"][900], world["prep"]["GICP"], world["T"]
    reg = registration(sp, case)
    with pytest.raises(sp.SpError) as e:
        reg.align_batch(S, prep, [], [case["scale"]])
    assert e.value.code == _lib.SP_ERR_INVALID_ARGUMENT and "batch must be in 1..SP_ALIGN_BATCH_MAX" in str(e.value)
    # a source of SP_ALIGN_BATCH_MAX_POINTS + 1 points
    big = sp.PointCloudShared(dev(np.tile(world["host"][900][0], (19, 1))[:16385]), covs=dev(np.tile(world["host"][900][1], (19, 1))[:16385]))
    assert big.size() == 16385
    with pytest.raises(sp.SpError) as e:
        sp.Registration(reg.params).align_batch(big, prep, [T["small"], T["large"]], [case["scale"]])
    assert e.value.code == _lib.SP_ERR_INVALID_ARGUMENT and "SP_ALIGN_BATCH_MAX_POINTS" in str(e.value)
    # a workspace one byte short, and a target without certificates
    good = reg.align_batch(S, prep, [T["small"], T["large"]], [case["scale"]])
    L = _lib.lib()
    T_dev, res_dev, _, ws = reg._batch_bufs
    before = res_dev.clone()
    fp, op, sc = reg._factor_params(case["scale"]), reg.opt_params(), (C.c_float * 1)(case["scale"])
    call = lambda target, nbytes: L.sp_gicp_align_batch(target, reg._psrc._h, sp._ptr(T_dev), sp._ptr(T_dev), 2, C.byref(fp), C.byref(op),  # noqa: E731
                                                        sc, 1, sp._ptr(res_dev), sp._ptr(ws), nbytes, sp._stream())
    assert call(prep._h, L.sp_gicp_align_batch_workspace_bytes(900, 2) - 1) == _lib.SP_ERR_INVALID_ARGUMENT
    assert b"workspace too small" in L.sp_last_error()
    plain = C.c_void_p()
    sp.check(L.sp_gicp_target_create_plain(prep.grid._h, sp._ptr(prep.covs), prep.covs.shape[0], sp._stream(), C.byref(plain)))
    try:
        assert call(plain, ws.numel()) == _lib.SP_ERR_INVALID_ARGUMENT
        assert b"no reuse certificates" in L.sp_last_error()
    finally:
        L.sp_gicp_target_destroy(plain)
    torch.cuda.synchronize()
    assert torch.equal(res_dev, before) and len(good) == 2  # nothing was enqueued


def test_cpp_facade(sp):
    exe = build(os.path.join(CPP, "test_align_batch.cpp"), os.path.join(CPP, "test_align_batch"))
    r = subprocess.run([exe, GOLD], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
    for name in ("batch_on_the_device", "sequential_fallback"):
        assert f"[  OK  ] {name}" in r.stdout, name
