"""`python bench.py --gpus N` with no launcher around it: the parent starts N ranks itself. The
children here are a stub (no GPU, no torch): what is under test is the launcher — ranks, environment, one line on stdout,
exit codes, and that a dead rank takes the waiting ones with it. Below them: bench.py's own options and output dump on the
host, and one GPU test that runs bench.py itself in its plain and --full forms."""
import io
import json
import os
import subprocess
import sys
import textwrap
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stub(tmp_path, body):
    p = tmp_path / "stub_main.py"
    p.write_text(textwrap.dedent(body))
    return [sys.executable, str(p)]


def test_launcher_starts_n_ranks_and_relays_rank0_line(tmp_path):
    import bench

    cmd = _stub(tmp_path, """
        import json, os, sys
        rank = int(os.environ["RANK"])
        open(os.path.join(os.path.dirname(__file__), f"rank{rank}.json"), "w").write(json.dumps(
            {k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                            "HSA_ENABLE_IPC_MODE_LEGACY")} | {"argv": sys.argv[1:]}))
        print(json.dumps({"metric": "stub", "rank": rank, "n_gpus": int(os.environ["WORLD_SIZE"])}))
        print("noise on stderr", file=sys.stderr)
    """)
    out = io.StringIO()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    rc = bench.launch_ranks(2, ["--gpus", "2", "--steps", "3"], child_cmd=cmd, env=env, stdout=out)
    assert rc == 0
    lines = [l for l in out.getvalue().splitlines() if l.strip()]
    assert len(lines) == 1  # ONE JSON line: rank 0's; rank 1's stdout goes nowhere
    assert json.loads(lines[0]) == {"metric": "stub", "rank": 0, "n_gpus": 2}
    seen = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(2)]
    for r, e in enumerate(seen):
        assert e["RANK"] == str(r) and e["LOCAL_RANK"] == str(r) and e["WORLD_SIZE"] == "2"
        assert e["MASTER_ADDR"] == "127.0.0.1" and e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
        assert e["argv"] == ["--gpus", "2", "--steps", "3"]
    assert seen[0]["MASTER_PORT"] == seen[1]["MASTER_PORT"] and int(seen[0]["MASTER_PORT"]) > 0


def test_launcher_reports_a_failed_rank_and_stops_the_others(tmp_path):
    import bench

    cmd = _stub(tmp_path, """
        import os, sys, time
        if os.environ["RANK"] == "1":
            sys.exit(3)
        time.sleep(600)  # rank 0 "waits in a collective" for the dead rank
    """)
    out = io.StringIO()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    t0 = time.time()
    rc = bench.launch_ranks(2, [], child_cmd=cmd, env=env, stdout=out)
    assert rc == 3 and time.time() - t0 < 60 and out.getvalue().strip() == ""


def test_bench_cli_takes_the_launcher_only_without_world_size(tmp_path):
    """Under torchrun (WORLD_SIZE set) the command behaves as before: no children. Without it, --gpus 2 goes through
    launch_ranks — checked on the real command line with the child command replaced by a stub through a wrapper."""
    wrapper = tmp_path / "run_bench_main.py"
    wrapper.write_text(textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import bench
        calls = []
        bench.launch_ranks = lambda n, argv, **kw: calls.append((n, argv)) or 0
        sys.argv = ["bench.py"] + sys.argv[1:]
        try:
            bench.main()
        except SystemExit as e:
            print("EXIT", e.code, calls)
    """))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(wrapper), "--gpus", "2", "--steps", "5"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert "EXIT 0 [(2, ['--gpus', '2', '--steps', '5'])]" in r.stdout, r.stdout + r.stderr


def test_repeats_defaults_to_one_block_and_to_31_with_full(monkeypatch):
    """Parsed options only: a plain run times ONE block of --steps steps, --full the median of 31, --repeats overrides
    either, --dump-outputs takes a folder. What main() does with them is checked on the GPU (test_bench_runs_on_the_gpu)."""
    import bench

    def parse(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return bench.parse()

    a = parse("--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.full, a.repeats, a.steps, a.warmup, a.dump_outputs) == (False, 1, 7, 3, None)
    a = parse("--full", "--dump-outputs", "outs")
    assert (a.full, a.repeats, a.dump_outputs) == (True, 31, "outs")
    assert parse("--full", "--repeats", "3").repeats == 3 and parse("--repeats", "5").repeats == 5


def test_dump_outputs_writes_what_the_caller_receives(tmp_path, monkeypatch):
    """bench.dump_outputs on host tensors standing in for the device buffers: one .npy per array, float32 / float64 only,
    the 192-byte linear system unpacked as Registration._read_lin unpacks it and the pose as Registration.T_from_device."""
    import numpy as np
    import torch

    import bench
    from sycl_points_amd.api import Registration

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)

    class Reg:  # the attributes of Registration that dump_outputs reads, on the host
        _lin = torch.arange(48, dtype=torch.float32)
        _iters_dev = torch.tensor([7], dtype=torch.int32)
        _read_lin = staticmethod(Registration._read_lin)
        T_from_device = staticmethod(Registration.T_from_device)

    Reg._lin[43] = 0.0
    Reg._lin.view(torch.int32)[43] = 123456  # inlier: a uint32 in the float buffer
    T_dev = torch.arange(16, dtype=torch.float32)
    delta = torch.linspace(0.0, 1.0, 8)
    bench.dump_outputs(str(tmp_path / "d"), Reg(), T_dev, delta)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert sorted(got) == ["H", "T", "b", "delta", "error", "inlier", "iterations"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["T"], np.arange(16, dtype=np.float32).reshape(4, 4).T)
    np.testing.assert_array_equal(got["H"], np.arange(36, dtype=np.float32).reshape(6, 6))
    np.testing.assert_array_equal(got["b"], np.arange(36, 42, dtype=np.float32))
    assert got["error"].tolist() == [42.0] and got["inlier"].tolist() == [123456.0] and got["iterations"].tolist() == [7.0]
    np.testing.assert_array_equal(got["delta"], delta.numpy())


@pytest.mark.gpu
def test_bench_runs_on_the_gpu(tmp_path):
    """bench.py itself at a small size: a plain run times one block of exactly --steps steps, runs none of the --full legs
    and dumps the last step's arrays, the same on a second run; --full times --repeats blocks and fills the other entries."""
    import numpy as np

    def run(*argv):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--points", "20000", *argv],
                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])

    plain = [run("--steps", "13", "--warmup", "3", "--dump-outputs", str(tmp_path / f"d{i}")) for i in range(2)]
    for d in plain:
        assert d["steps"] == 13 and d["warmup"] == 3 and d["full"] is False and d["timed_blocks"]["n"] == 1
        assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "correspondences/s" and d["dtype"] == "f32"
        for key in ("kernels", "roofline", "launches_of_one_alignment", "until_converged", "stages",
                    "pose_max_abs_err_vs_ground_truth"):
            assert d[key] is None, key
        assert "cpu_baseline" not in d
    a = {p.stem: np.load(p) for p in (tmp_path / "d0").iterdir()}
    b = {p.stem: np.load(p) for p in (tmp_path / "d1").iterdir()}
    assert sorted(a) == sorted(b) == ["H", "T", "b", "delta", "error", "inlier", "iterations"]
    assert a["iterations"].tolist() == [13.0]  # 13 steps: one call of 13 iterations (alignments are 20 long)
    assert np.isfinite(a["T"]).all() and a["inlier"][0] > 0
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6, err_msg=k)

    full = run("--steps", "20", "--warmup", "3", "--full", "--repeats", "2", "--no-stages", "--no-cpu-baseline")
    assert full["full"] is True and full["timed_blocks"]["n"] == 2
    for key in ("kernels", "roofline", "launches_of_one_alignment", "until_converged"):
        assert full[key] is not None, key
    assert full["pose_max_abs_err_vs_ground_truth"] < 1e-3
