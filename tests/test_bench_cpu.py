"""bench.py contract on CPU: ``--gpus N`` launches N ranks itself (no torchrun), rank 0 prints ONE JSON
line that reports the real world size and the engines' collective traffic; a WORLD_SIZE that disagrees
with ``--gpus`` is refused (reference launch patterns: Stoke-DDP.py:2, Fairscale-DDP.py:125-132)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(OMP_NUM_THREADS="2", **kw)
    return env


def test_bench_self_launches_two_gloo_ranks():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--workload", "resnet18-cpu", "--steps", "1",
                        "--warmup", "1", "--micro-batch", "2"], cwd=ROOT, env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_ranks"] == 2
    assert res["config"]["parallelism"] == "dp2"
    assert res["config"]["global_batch"] == 4
    # DDP gradient buckets + the clip-norm scalar cross the wire every step
    assert res["collectives_per_step"] >= 2
    assert res["comm_bytes_per_step"] >= 4 * 11_000_000


def test_bench_world2_reports_topology_and_secondary_headline():
    """Both BASELINE headlines at every N (the ResNet DDP one as 'secondary'), with the c10d world size read
    back from the process group and every rank's device in 'topology'."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--device", "cpu", "--workload", "gpt2-fsdp",
                        "--model", "gpt2-tiny", "--micro-batch", "2", "--seq", "64", "--steps", "2", "--warmup", "1",
                        "--secondary-micro-batch", "2", "--full"], cwd=ROOT, env=_env(), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["config"]["parallelism"] == "fsdp2" and res["collectives_per_step"] > 0
    topo = res["topology"]
    assert topo["c10d_world"] == 2 and topo["c10d_backend"] == "gloo"
    assert [d["rank"] for d in topo["devices"]] == [0, 1]
    sec = res["secondary"]
    assert sec["config"]["parallelism"] == "dp2" and sec["value"] > 0
    assert sec["collectives_per_step"] >= 2


def test_bench_under_torchrun_driver_command():
    """The driver's own launch form for N > 1 (torch.distributed.run, one rank per device, env:// on 127.0.0.1):
    exactly one JSON line from rank 0 with the real world size."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2",
                        "--device", "cpu", "--workload", "gpt2-fsdp", "--model", "gpt2-tiny", "--micro-batch", "2",
                        "--seq", "64", "--steps", "2", "--warmup", "1", "--secondary-micro-batch", "2", "--full"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_ranks"] == 2 and res["topology"]["c10d_world"] == 2 and res["steps"] == 2
    assert res["secondary"]["config"]["parallelism"] == "dp2"


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--device", "cpu", "--workload", "gpt2-fsdp",
                        "--model", "gpt2-tiny", "--micro-batch", "2", "--seq", "64", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out_dir], cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


def test_bench_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """A plain run times --steps steps and nothing else (no 'secondary': that is behind --full), reports
    ms_per_step, and --dump-outputs writes the last timed step's loss and parameter sample as float32 .npy
    files that a second run with the same arguments reproduces exactly."""
    import numpy as np
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    res, err = _plain_run(a)
    assert "secondary" not in res and "secondary_error" not in res
    assert err.count("warmup step 0 done") == 1      # one measurement ran, not two
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0 and res["unit"] == "tokens/s" and res["higher_is_better"] is True
    assert abs(res["value"] - 2 * 64 / (res["ms_per_step"] / 1000)) <= 1e-3 * res["value"]
    _plain_run(b)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["loss.npy", "params_sample.npy"]
    total = 0
    for name in os.listdir(a):
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all()
        assert np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 * 1024 * 1024
    loss = float(np.load(os.path.join(a, "loss.npy"))[0])
    assert 0.0 < loss < 20.0


def test_bench_param_sample_is_fixed_and_bounded():
    """The parameter sample of --dump-outputs: everything when it fits, else the same k positions every time."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    ts = [torch.arange(0, 7, dtype=torch.float64), torch.arange(7, 30).reshape(23, 1).bfloat16(), torch.arange(30, 41)]
    whole = bench.sample_flat(ts, k=41)
    assert whole.dtype == torch.float32 and whole.tolist() == list(range(41))
    s1, s2 = bench.sample_flat(ts, k=16), bench.sample_flat(ts, k=16)
    assert s1.numel() == 16 and torch.equal(s1, s2)
    assert s1.tolist() == sorted(s1.tolist()) and set(s1.tolist()) <= set(range(41))
    assert bench.DUMP_PARAM_SAMPLE * 4 <= 64 * 1024 * 1024


def test_bench_refuses_mismatched_world_size():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--workload", "resnet18-cpu"], cwd=ROOT,
                       env=_env(WORLD_SIZE="2"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "WORLD_SIZE=2" in r.stderr


def test_bench_secondary_failure_on_one_rank_keeps_primary_line():
    """a failure of the secondary ResNet measurement on ONE rank must not strand the other rank in
    a DDP collective: the ranks agree at the guarded phase boundaries, skip the secondary together, and rank 0
    still prints the primary GPT-2 line (with the reason in 'secondary_error')."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--device", "cpu", "--workload", "gpt2-fsdp",
                        "--model", "gpt2-tiny", "--micro-batch", "2", "--seq", "64", "--steps", "1", "--warmup", "1",
                        "--secondary-micro-batch", "2", "--full"], cwd=ROOT, env=_env(PDT_BENCH_SECONDARY_FAIL_RANK="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["config"]["parallelism"] == "fsdp2" and res["value"] > 0
    assert "secondary" not in res
    assert "injected secondary failure" in res["secondary_error"] or "another rank" in res["secondary_error"]


def test_headline_guard_refuses_shared_gpus():
    """A GPU run at N > 1 prints a headline only when c10d world == --gpus == distinct devices."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dev = types.SimpleNamespace(type="cuda")
    args = types.SimpleNamespace(gpus=4)
    good = {"metric": "m", "topology": {"c10d_world": 4, "distinct_devices": 4}}
    assert bench.headline_ok(good, args, dev, 4)
    shared = {"metric": "m", "topology": {"c10d_world": 4, "distinct_devices": 1}}
    assert not bench.headline_ok(shared, args, dev, 4)
    wrong_world = {"metric": "m", "topology": {"c10d_world": 2, "distinct_devices": 2}}
    assert not bench.headline_ok(wrong_world, args, dev, 4)
    old = os.environ.get("PDT_BENCH_REHEARSAL")
    os.environ["PDT_BENCH_REHEARSAL"] = "1"
    try:
        assert bench.headline_ok(shared, args, dev, 4) and shared["rehearsal"] and "REHEARSAL" in shared["metric"]
    finally:
        if old is None:
            del os.environ["PDT_BENCH_REHEARSAL"]
        else:
            os.environ["PDT_BENCH_REHEARSAL"] = old
    assert bench.headline_ok({"metric": "m", "topology": {}}, types.SimpleNamespace(gpus=1), dev, 1)
