"""The N>1 path: units shard across ranks with no data-path collective; one config broadcast at start.
Exercised with world_size-2 gloo on the CPU (the partition + broadcast logic of srslte_amd.sharding)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, sys, json
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from srslte_amd import sharding
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
cfg = sharding.broadcast_config({"n_prb": 100, "n_fft": 2048, "k_cb": 6144, "nit": 8} if dist.get_rank() == 0 else None)
lo, hi = sharding.shard_range(1001, dist.get_rank(), dist.get_world_size())
t = sharding.max_over_ranks(float(dist.get_rank() + 1))
print(json.dumps({"rank": dist.get_rank(), "cfg": cfg, "lo": lo, "hi": hi, "t": t}), flush=True)
dist.destroy_process_group()
"""


def test_world_size_2_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    import json
    res = sorted((json.loads(o.strip().splitlines()[-1]) for o in outs), key=lambda d: d["rank"])
    assert res[0]["cfg"] == res[1]["cfg"] == {"n_prb": 100, "n_fft": 2048, "k_cb": 6144, "nit": 8}
    assert (res[0]["lo"], res[0]["hi"], res[1]["lo"], res[1]["hi"]) == (0, 501, 501, 1001)
    assert res[0]["t"] == res[1]["t"] == 2.0


def test_shard_range_partitions_exactly():
    from srslte_amd import sharding

    for n in (0, 1, 7, 64, 1001):
        for w in (1, 2, 3, 8):
            parts = [sharding.shard_range(n, r, w) for r in range(w)]
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[i][1] == parts[i + 1][0] for i in range(w - 1))
            assert max(h - l for l, h in parts) - min(h - l for l, h in parts) <= 1


def test_bench_launcher_world_size_2_end_to_end():
    """`python bench.py --gpus 2` from a plain interpreter: the parent spawns the two ranks itself (no torchrun), they rendezvous
    on 127.0.0.1 (gloo in this GPU-less rehearsal), broadcast the configuration, take their shard, and rank 0 prints ONE JSON line
    with n_gpus 2.  --plumbing-only runs no kernels: on the GPU box the same launcher starts the real workers."""
    import json

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--sf", "101",
                        "--plumbing-only"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["steps"] == 3 and r["plumbing_only"] is True
    assert r["config"] == {"n_prb": 100, "n_fft": 2048, "k_cb": 6144, "nit": 8, "cb_per_sf": 13, "sf": 101}
    assert [tuple(s) for s in r["shards"]] == [(0, 101), (101, 202)]  # weak scaling: the unit list grows with the world size
    assert r["max_step_time_s"] >= 0.02  # the slowest rank (rank 1 sleeps 20 ms) sets the time


def test_bench_launcher_propagates_a_failing_rank():
    """a rank that dies must fail the whole run (non-zero exit, no JSON line), not leave the others waiting in a barrier"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    # --gpus 2 without --plumbing-only on a box without GPUs: every worker exits with "needs a HIP device"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    import torch

    if not torch.cuda.is_available():
        assert p.returncode != 0 and not [l for l in p.stdout.splitlines() if l.startswith("{")]
    # a worker launched with a world size that contradicts --gpus refuses to run
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plumbing-only"],
                       env=dict(env, RANK="0", WORLD_SIZE="3", LOCAL_RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode != 0 and "does not match WORLD_SIZE" in p.stderr


AGREE_WORKER = r"""
import os, sys, json
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from srslte_amd import sharding
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
label, dev = sharding.init_collectives(rank, world, torch.device("cpu"), prefer="nccl", timeout_s=60)
cfg = sharding.broadcast_config({"k_cb": 6144} if rank == 0 else None, dev)
seen = sharding.ranks_seen(rank, None, dev)
t = sharding.max_over_ranks(float(rank + 1), dev)
line = json.dumps({"rank": rank, "label": label, "cfg": cfg, "seen": seen, "t": t, "backend": dist.get_backend()}) + "\n"
# the ranks may share one pipe (torch.distributed.run): the line and its newline go out in ONE write, which a pipe keeps whole below PIPE_BUF -- print()
# on an unbuffered stdout writes the newline by itself, and another rank's line can land in front of it
assert len(line) < 4096
sys.stdout.flush()
os.write(1, line.encode())
dist.destroy_process_group()
"""


def _run_agree(tmp_path, world):
    import json

    script = tmp_path / "agree.py"
    script.write_text(AGREE_WORKER % ROOT)
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-1500:] for o in outs]
    return sorted((json.loads([l for l in o[0].splitlines() if l.startswith("{")][-1]) for o in outs), key=lambda d: d["rank"])


def test_collective_backend_is_agreed_by_all_ranks(tmp_path):
    """no GPU here, so the RCCL attempt fails on BOTH ranks: they must hear of each other's failure through the rendezvous store, rebuild
    the group on gloo over the same store (no second port) and say so -- nobody stays behind on the other backend, nobody waits for a timeout"""
    import time

    import torch

    if torch.cuda.is_available():
        import pytest

        pytest.skip("needs a box where RCCL cannot come up")
    t0 = time.time()
    res = _run_agree(tmp_path, 2)
    assert time.time() - t0 < 60
    for r in res:
        assert r["backend"] == "gloo" and r["label"].startswith("gloo (RCCL failed on ranks [0, 1]"), r
        assert r["cfg"] == {"k_cb": 6144} and r["t"] == 2.0
        assert [x["rank"] for x in r["seen"]] == [0, 1]


def test_collectives_are_initialised_at_world_size_1(tmp_path):
    """a 1-rank job builds its process group too (on the GPU box: RCCL at world size 1; here: the agreed fallback)"""
    res = _run_agree(tmp_path, 1)
    assert len(res) == 1 and res[0]["cfg"] == {"k_cb": 6144} and res[0]["t"] == 1.0 and len(res[0]["seen"]) == 1


def test_collectives_under_torch_distributed_run(tmp_path):
    """the driver starts N > 1 ranks with `python -m torch.distributed.run --master-addr 127.0.0.1 --master-port P`: the elastic agent
    then OWNS that port (TORCHELASTIC_USE_AGENT_STORE=True) and every rank, 0 included, must join its store as a client
    (sharding.job_store) -- a second server on the port is EADDRINUSE on rank 0 (round-3 advice)"""
    import json
    import socket

    script = tmp_path / "agree.py"
    script.write_text(AGREE_WORKER % ROOT)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = sorted((json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [r["rank"] for r in res] == [0, 1]
    for r in res:
        assert r["cfg"] == {"k_cb": 6144} and r["t"] == 2.0 and [x["rank"] for x in r["seen"]] == [0, 1]


def test_bench_worker_under_torch_distributed_run():
    """bench.py itself as the driver launches it for N > 1 (plumbing rehearsal: no kernels)"""
    import json
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--sf", "11", "--plumbing-only"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and [tuple(x) for x in r["shards"]] == [(0, 11), (11, 22)]
