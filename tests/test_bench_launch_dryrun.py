"""bench.py under the driver's launcher (`python -m torch.distributed.run --nproc-per-node 2 ...`)
with the no-compute stand-in library: proves the N > 1 launch contract end to end on CPU --
RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* parsing, the unique-id rendezvous next to the launcher's own
store, barrier/max-over-ranks plumbing, exactly ONE JSON line from rank 0."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_lib(tmp_path):
    so = str(tmp_path / "libfake_msegk.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-w", "-o", so, os.path.join(HERE, "fake_msegk.c")])
    return so


def test_bench_two_ranks_prints_one_json_line(tmp_path):
    env = dict(os.environ, MSK_FAKE_LIB=_fake_lib(tmp_path), OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "run_bench_fake.py"), "--gpus", "2",
           "--steps", "2", "--warmup", "1", "--size", "16", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["scaling"] == "weak"
    assert rec["config"]["global_batch"] == 4 and rec["config"]["parallelism"] == "dp2"
    assert rec["unit"] == "voxels/s" and rec["higher_is_better"] is True and "roofline" in rec
    assert "cpu_baseline" not in rec                         # rank 0 at N=1 only
    # round 4: the first multi-GPU run must be diagnosable from the line alone
    # round 5: the default arrangement is decided from the communication budget -- `--dp-mode auto` = overlapped buckets (mode 2)
    # whenever there is more than one rank -- and the line carries the exposed communication (step minus a compute-only replay)
    dp = rec["dp"]
    assert dp["dp_mode_requested"] == "auto" and dp["dp_mode"] == 2 and dp["overlap_buckets"] is True and dp["buckets_last_step"] >= 2
    assert "exposed_comm_ms_per_step" in dp and len(dp["compute_only_ms_per_step_per_rank"]) == 2
    assert rec["config"]["eager_optimizer"] is False          # gradients are final only after the all-reduce
    assert len(dp["allreduce_busbw_GBps_per_rank"]) == 2 and len(dp["syncbn_collective_ms_per_step_per_rank"]) == 2
    assert set(dp["per_rank_collective_ms_per_step"]) == {"rccl_allreduce", "rccl_allreduce_stats", "rccl_allgather", "rccl_allreduce_bucket"}
    assert rec["roofline"]["strict_fp32"] is None            # the exact-operand pass is a 1-GPU extra
    # --dp-mode 0: ONE all-reduce after backward, everything on the compute stream
    cmd2 = cmd[:cmd.index(os.path.join(HERE, "run_bench_fake.py"))]
    cmd2[cmd2.index("--master-port") + 1] = str(_free_port())
    cmd2 += [os.path.join(HERE, "run_bench_fake.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--size", "16", "--no-cpu-baseline",
             "--dp-mode", "0"]
    out2 = subprocess.run(cmd2, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out2.returncode == 0, out2.stderr[-2000:]
    rec2 = json.loads([l for l in out2.stdout.splitlines() if l.startswith("{")][0])
    assert rec2["dp"]["dp_mode"] == 0 and rec2["dp"]["overlap_buckets"] is False and rec2["dp"]["buckets_last_step"] == 1


def test_bench_plain_python_gpus_2_spawns_its_own_ranks(tmp_path):
    """round-4 verdict, Weak 9: `python bench.py --gpus 2` with NO launcher (WORLD_SIZE unset) must not die on the launch
    contract -- it becomes the launcher (parallel.spawn_ranks: one process per GPU, own rendezvous) and rank 0 prints the line."""
    env = dict(os.environ, MSK_FAKE_LIB=_fake_lib(tmp_path), OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "run_bench_fake.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--size", "16", "--no-cpu-baseline"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 4 and rec["config"]["parallelism"] == "dp2"
    assert rec["dp"]["dp_mode"] == 2 and len(rec["dp"]["per_rank_step_ms"]) == 2
    # a rank that fails takes the job down with a non-zero exit code instead of leaving its peers in the rendezvous
    bad = subprocess.run([sys.executable, os.path.join(HERE, "run_bench_fake.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--size", "16", "--no-cpu-baseline", "--opt", "broken"], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert bad.returncode != 0


def test_bench_single_process_defaults(tmp_path):
    env = dict(os.environ, MSK_FAKE_LIB=_fake_lib(tmp_path))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "run_bench_fake.py"), "--steps", "1", "--warmup", "0",
                          "--size", "16", "--no-cpu-baseline"], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(out.stdout.strip().splitlines()) == 1, out.stdout[:500]     # ONE line on stdout: log messages go to stderr
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert rec["n_gpus"] == 1 and rec["dtype"] == "f32" and rec["data"] == "synthetic" and rec["vs_baseline"] is None
    assert rec["config"]["eager_optimizer"] is True
    # a launcher that provided FEWER ranks than --gpus asks for is an error, not a silent smaller run
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    bad = subprocess.run([sys.executable, os.path.join(HERE, "run_bench_fake.py"), "--gpus", "2", "--size", "16"],
                         env=env2, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: the last timed step's outputs as float .npy files under 64 MB in all, the same on every run with the same
    arguments; --steps is the number of timed steps and the line carries ms_per_step."""
    import numpy as np
    env = dict(os.environ, MSK_FAKE_LIB=_fake_lib(tmp_path), OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        out = subprocess.run([sys.executable, os.path.join(HERE, "run_bench_fake.py"), "--steps", "3", "--warmup", "1",
                              "--size", "16", "--no-cpu-baseline", "--dump-outputs", str(d)], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        assert len(out.stdout.strip().splitlines()) == 1, out.stdout[:500]
        rec = json.loads(out.stdout)
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        assert rec["roofline"]["event_steps"] == 1 and "3 timed steps" in rec["roofline"]["events"]   # every 4th of 3 steps
        files = sorted(os.listdir(d))
        assert files == sorted(n + ".npy" for n in rec["dump_outputs"]["elements_stored_of_total"])
        assert {"loss.npy", "loss_terms.npy", "per_channel_dice.npy", "logits.npy", "state.npy"} <= set(files)
        assert sum(os.path.getsize(d / f) for f in files) <= 64 * 10 ** 6
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["logits.npy"].shape == (2, 3, 16, 16, 16)                            # small enough to be stored whole
        stored, total = rec["dump_outputs"]["elements_stored_of_total"]["state"]
        assert stored == arrays["state.npy"].size < total and np.abs(arrays["state.npy"]).max() > 0   # a seeded sample
        dumps.append(arrays)
    for f, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][f]), f
    bad = subprocess.run([sys.executable, os.path.join(HERE, "run_bench_fake.py"), "--steps", "0", "--size", "16"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0
