"""bench.py plumbing on one GPU, so that the first real multi-GPU run cannot fail on anything but the hardware:
the N = 2 launch exactly as the driver does it (`python -m torch.distributed.run ... bench.py --gpus 2`), with
BENCH_BACKEND=gloo so that both ranks can share GPU 0 (RCCL needs one device per rank), at small sizes; the JSON
line must carry the contract's keys and the parity assertions of the sharded legs must have run.  N > 1 numbers
themselves are NOT measured anywhere in this repository's own runs (one GPU per gpurun box)."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config", "roofline")


def _last_json_line(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert lines, text[-2000:]
    return json.loads(lines[-1])


def test_bench_plain_run_times_the_steps_and_dumps_the_result(tmp_path):
    """A plain run: the contract's keys, nothing of --full, and --dump-outputs holds the last step's result exactly:
    sum_i s_i [t_i]G = [sum_i s_i t_i]G for the seeded inputs bench.py makes (t_i, s_i: its SplitMix vectors)."""
    import ctypes

    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from bellman_amd import _lib
    from oracle import cref

    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--log-n", "12",
                        "--dump-outputs", str(dump)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = _last_json_line(r.stdout)
    for k in CONTRACT_KEYS:
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    for k in ("cpu_baseline", "msm_boolean_heavy", "fft", "create_proof", "scaling_model"):
        assert k not in out, k
    assert out["config"]["value_with_2_jobs_in_flight"] is None and out["config"]["value_classic_plan_no_table_per_gpu"] is None
    got = np.load(dump / "msm_result.npy")
    assert got.dtype == np.float64 and got.shape == (2, 12)
    n = 1 << 12
    k = np.array(cref.int_to_limbs(cref.fr_dot(bench.splitmix_scalars(n, 0x5CA1A25), bench.splitmix_scalars(n, 0x62656C6C6D616E)), 4),
                 dtype=np.uint64)
    want = np.zeros(12, dtype=np.uint64)
    _lib.load().bh_point_mul(1, want.ctypes.data_as(ctypes.c_void_p), bench.G1_GEN_MONT.ctypes.data_as(ctypes.c_void_p),
                             k.ctypes.data_as(ctypes.c_void_p))
    assert np.array_equal(got, want.view(np.uint32).reshape(2, 12).astype(np.float64))


def test_bench_single_gpu_contract_small():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--log-n", "12", "--no-proof", "--full"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = _last_json_line(r.stdout)
    for k in CONTRACT_KEYS + ("cpu_baseline",):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["unit"] == "Mscalar-mul/s" and out["value"] > 0 and out["vs_baseline"] is None
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(out["roofline"])
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(out["cpu_baseline"])
    assert "workload" in out["config"] and "model" not in out["config"]
    # [r6] what the launch executed is reported, not assumed: additions counted on the device, the plan they ran under
    alu = out["roofline"]["alu"]
    assert 0 < alu["mixed_additions_per_launch"] <= alu["sorted_entries"] - alu["zero_digits"]
    assert alu["plan"]["window_bits"] > 0 and alu["plan"]["chunk"] > 0


def test_bench_scaling_model_is_emitted():
    """[r6] the N = 1 line carries the predicted 1 / 2 / 4 / 8-rank table of DESIGN.md 7 (one rank's share measured on this
    GPU), at reduced sizes here"""
    sys.path.insert(0, ROOT)
    import bellman_amd
    import bench
    from bellman_amd import _lib

    w = bellman_amd.Worker(0)
    m = bench.bench_scaling_model(w, _lib.load(), log_n_total=16, proof_log_n=12, reps=2)
    w.close()
    for leg in ("msm_2p16_strong", "proof_2p12_strong"):
        assert set(m[leg]) == {"1", "2", "4", "8"}
        assert all(m[leg][k]["predicted_ms"] > 0 and m[leg][k]["predicted_speedup"] > 0 for k in m[leg])
    assert m["msm_2p16_strong"]["8"]["terms_per_rank"] == 1 << 13


@pytest.mark.parametrize("ranks", [2, 8])
def test_bench_ranks_on_one_gpu_gloo(ranks):
    """2 ranks, and the 8 ranks of the driver's full-node run (rank-count-dependent splits of the C5 legs)"""
    env = dict(os.environ, BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(29517 + ranks), "bench.py", "--gpus", str(ranks), "--steps", "2", "--warmup", "1", "--log-n", "12",
           "--proof-log-n", "10", "--c5-log-n", "13", "--check-log-n", "10", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = _last_json_line(r.stdout)
    for k in CONTRACT_KEYS:
        assert k in out, k
    assert out["n_gpus"] == ranks and out["scaling"] == "weak" and out["value"] > 0
    # the parity assertions of the N > 1 legs ran (they raise inside bench.py otherwise)
    assert "== one multiexp" in out["sharded_fold_check"]
    assert out["create_proof_sharded"]["scaling"] == "strong" and "identical to the single-GPU proof" in out["create_proof_sharded"]["workload"]
    assert out["msm_c5_sharded"]["scaling"] == "strong" and out["msm_c5_sharded"]["value"] > 0
    # [r6] the line judges itself against the scaling model of DESIGN.md 7: predicted (slowest shard alone + collective) next to measured
    model = out["msm_c5_sharded"]["model"]
    assert model["predicted_ms"] > 0 and model["measured_ms"] > 0
    assert "cpu_baseline" not in out          # rank 0 at N = 1 only
    # [r4] the line proves who ran: every rank reported in, here all of them on the one GPU of the box (under RCCL
    # bench.py asserts distinct_devices == world itself)
    assert out["ranks_seen"] == ranks and out["distinct_devices"] == 1 and len(out["ms_per_step_per_rank"]) == ranks
    assert [r["rank"] for r in out["ranks"]] == list(range(ranks)) and out["backend"].startswith("gloo")
    assert out["library"]["version"].startswith("bellman_hip") and not out["library"]["override"]
    assert out["msm_one_process_sharded"]["contexts"] == ranks and out["msm_one_process_sharded"]["value"] > 0
