"""The N > 1 path of bench.py on the one-GPU box: every line of the multi-rank rank body -- process
group, shard, all-reduce of the gradient sums, barrier + max-over-ranks timing, per-rank gather -- runs under the driver's
`-m gpu` suite, so BASELINE configs[3] (8 x configs[2], sharding argument /root/reference/model.py:260, 267) is one
command away from a tested state.  The launcher starts the ranks as child processes before this process's GPU use matters
(bench.py never execs and never touches the GPU in the parent)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--bond-dim", "32", "--T", "600", "--batch-per-gpu", "16", "--no-cpu-baseline"]


def _bench(args, timeout=600, json_lines=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert lines and len(lines[-1]) < 4096, proc.stdout[-2000:]           # the contract's record: last line, compact
    assert all('"detail"' in l[:12] for l in lines[:-1]), proc.stdout[-2000:]
    if json_lines is not None:
        assert len(lines) == json_lines, proc.stdout[-2000:]
    return json.loads(lines[-1])


def test_two_rank_rehearsal_on_one_gpu():
    """`bench.py --gpus 2 --rehearse-on-one-gpu`: two child ranks that share cuda:0 and all-reduce over gloo."""
    rec = _bench(["--gpus", "2", "--rehearse-on-one-gpu", "--full", "--steps", "2", "--warmup", "1"] + SMALL)
    assert rec["n_gpus"] == 2 and rec["rccl_world_size"] == 2 and rec["collective_backend"] == "gloo"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["scaling"] == "weak"
    pr = rec["per_rank_ms_per_step"]
    assert 0.0 < pr["min"] <= pr["max"]
    assert rec["value"] > 0 and rec["ms_per_step"] >= pr["max"] * 0.999          # max over ranks, barrier included
    assert rec["config"]["parallelism"] == "dp2" and "global 32" in rec["config"]["workload"]
    assert "rehearsal" in rec and rec["cpu_baseline"] is None
    # one collective per step of 2 D^2 + 3 D + 2 floats, and every rank holds bit-identical variables and Adam slots after 3 steps
    # (the invariant configs[3] rests on: same all-reduced sums -> same update everywhere; /root/reference has no counterpart)
    assert rec["collective"]["message_bytes"] == 4 * (2 * 32 * 32 + 3 * 32 + 2) and rec["collective"]["calls_per_step"] == 1
    assert rec["collective"]["replicas_bit_identical_after_run"] is True
    # whole-job aggregate: both ranks' samples over the max-over-ranks time
    assert rec["value"] == pytest.approx(2 * 16 * 600 * 2 / (rec["ms_per_step"] * 2e-3), rel=1e-6)


def test_one_rank_through_rccl_matches_in_process():
    """`bench.py --gpus 1 --spawn`: one child rank with a real RCCL communicator (init with device_id, all-reduce of the
    gradient buffer on the device, barrier(device_ids), all_gather) against the in-process N = 1 run of the same shape."""
    # BASELINE configs[2] per GPU (the shape configs[3] runs on each of its 8 GPUs): an ~11 ms step, so that the one-rank
    # collective (~0.1 - 0.4 ms with its host hand-over) stays inside the tolerance
    shape = ["--no-cpu-baseline", "--steps", "6", "--warmup", "2"]
    spawned = _bench(["--gpus", "1", "--spawn"] + shape)
    inproc = _bench(["--gpus", "1"] + shape)
    assert spawned["n_gpus"] == 1 and spawned["collective_backend"] == "nccl" and spawned["rccl_world_size"] == 1
    assert spawned["collective"]["settings"]["NCCL_PROTO"] == "LL"          # the low-latency default is in force under RCCL
    assert spawned["allreduce_us"] is not None and 0.0 < spawned["allreduce_us"] < 5e4
    assert inproc["collective_backend"] is None and inproc["allreduce_us"] is None
    assert spawned["final_loss"] == pytest.approx(inproc["final_loss"], rel=1e-5)      # same parameters after the same steps
    assert spawned["value"] == pytest.approx(inproc["value"], rel=0.10), (spawned["value"], inproc["value"], spawned["allreduce_us"])


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """A plain run prints the record and nothing else (no kernel pass, roofline, CPU baseline or parity: those are --full's), and
    `--dump-outputs` writes what the last timed step computed.  The same arguments give the same inputs and the kernels are
    deterministic, so a second run writes the same bits."""
    D, T, B, K = 32, 600, 16, 3
    shape = ["--bond-dim", str(D), "--T", str(T), "--batch-per-gpu", str(B), "--steps", str(K), "--warmup", "1"]
    dumps = []
    for i in range(2):
        rec = _bench(shape + ["--dump-outputs", str(tmp_path / f"run{i}")], json_lines=1)
        assert rec["steps"] == K and rec["n_gpus"] == 1 and rec["detail_lines"] == []
        assert rec["roofline"] is None and rec["cpu_baseline"] is None and "parity_in_bench" not in rec
        assert rec["value"] == pytest.approx(B * T * K / (rec["ms_per_step"] * K * 1e-3), rel=1e-6)
        dumps.append({os.path.splitext(f)[0]: np.load(tmp_path / f"run{i}" / f) for f in os.listdir(tmp_path / f"run{i}")})
        d = dumps[-1]
        assert d["loss_per_clip"].shape == (B,) and d["grad_sums"].shape == (2 * D * D + 3 * D + 2,) and d["losses"].shape == (2,)
        assert d["var_Rx"].shape == (D, D) and d["adam_v_freqs"].shape == (D,) and len(d) == 3 + 3 * 6
        assert all(a.dtype == np.float32 and np.all(np.isfinite(a)) for a in d.values())
        assert float(d["losses"][0]) == pytest.approx(rec["final_loss"], rel=1e-9)        # the record keeps 10 digits
        assert d["grad_sums"][-1] == pytest.approx(float(np.sum(d["loss_per_clip"], dtype=np.float64)), rel=1e-5)
        assert float(d["losses"][0]) == pytest.approx(d["grad_sums"][-1] / B, rel=1e-5)
    assert dumps[0].keys() == dumps[1].keys()
    for k in dumps[0]:
        np.testing.assert_array_equal(dumps[0][k], dumps[1][k], err_msg=k)
