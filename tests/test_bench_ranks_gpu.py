"""GPU: bench.py's multi-rank path end to end (torchrun, 2 ranks).  Only one GPU is
available to the tests, so both ranks use cuda:0 and the collective runs over gloo; the
launch line, env handling, barrier / max-over-ranks timing, split-graph step and the JSON
contract are the real ones."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_json_contract():
    env = dict(os.environ, MSR3D_BENCH_SINGLE_DEVICE="1", MSR3D_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29671", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "4", "--warmup", "2", "--batch", "4", "--full"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]          # rank 0 prints ONE JSON line
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 4 and j["warmup"] == 2
    assert j["scaling"] == "weak" and j["higher_is_better"] is True
    assert j["config"]["global_batch"] == 8 and j["config"]["parallelism"] == "dp2"
    assert j["value"] > 0 and j["roofline"]["frac"] > 0
    assert "cpu_baseline" not in j                      # N=1 only
    # the line proves it was a 2-rank run: communicator size seen through a collective, the gradient
    # exchange timed on the communication stream, identical replicas afterwards
    c = j["comm"]
    assert c["ranks_seen"] == 2 and c["exchanges"] == 4 and c["allreduce_ms"] > 0
    assert c["allreduce_exposed_ms"] >= 0 and c["replica_checksum_spread"] == 0.0
    assert c["grad_bytes"] > 20e6 and c["exchange"] == "allreduce"


def test_bench_multi_rank_schedule_over_rccl_with_one_rank():
    """The multi-rank schedule on the REAL backend: RCCL communicator (one rank -- the box has one
    GPU), all-reduce of the flat gradient buffer on the communication stream between the replayed
    forward/backward graph and the optimiser, the next batch's encoder issued in between."""
    env = dict(os.environ, MSR3D_BENCH_FORCE_DIST="1", MASTER_PORT="29672", HSA_ENABLE_IPC_MODE_LEGACY="0",
               MSR3D_DP_GRAPH_COMM="0")           # (this test is about the eager-exchange schedule)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "3",
                          "--no-cpu-baseline", "--full"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["n_gpus"] == 1 and j["config"]["parallelism"] == "dp1"
    assert j["config"]["allreduce_hidden_behind_next_encoder"] is True and j["config"]["hip_graph"] is True
    assert j["value"] > 0 and j["roofline"]["launches"] >= 1 and j["census_us"]["msr3d_sa_level1_rows"][1] == 1.0
    assert j["comm"]["ranks_seen"] == 1 and j["comm"]["exchanges"] == 6 and j["comm"]["allreduce_ms"] > 0
    assert {"p10", "p50", "p90"} <= set(j["ms_per_step_percentiles"])


@pytest.mark.parametrize("micro_steps", [True, False])
def test_bench_reduce_scatter_all_gather_exchange_and_accumulation(micro_steps):
    """MSR3D_DP_EXCHANGE=rs_ag (the A/B switch for the 8-GPU run) on the one-rank RCCL communicator,
    with the reference's launch shape: 4 scenes x 5 accumulated micro-batches per optimiser step."""
    env = dict(os.environ, MSR3D_BENCH_FORCE_DIST="1", MASTER_PORT="29683" if micro_steps else "29673",
               HSA_ENABLE_IPC_MODE_LEGACY="0", MSR3D_DP_EXCHANGE="rs_ag", MSR3D_DP_GRAPH_COMM="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                          "--batch", "4", "--accum", "5", "--no-cpu-baseline", "--full"] +
                         (["--micro-steps"] if micro_steps else []), env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["comm"]["exchange"] == "rs_ag" and j["comm"]["exchanges"] == 3      # one per OPTIMISER step
    assert j["config"]["grad_accumulation"] == 5 and j["config"]["global_batch"] == 20
    assert j["config"]["window_step"] is (not micro_steps)
    assert j["census_us"]["msr3d_sa_level1_rows"][1] == 1.0 and j["value"] > 0     # one encoder pass per accumulation WINDOW


def test_bench_single_rank_json_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                          "--batch", "2", "--cpu-baseline-seconds", "1", "--full"], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert set(j["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    assert set(j["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample", "median_s_per_sample", "p10_s",
                                      "p90_s", "one_thread_value", "host"}
    assert j["vs_baseline"] is None and j["data"] == "synthetic"


def test_bench_default_line_carries_the_full_step_and_the_levels():
    """`--full` without workload flags: the headline line carries the roofline of the slowest SharedMLP level
    with all three levels beside it (distinct-row FLOPs priced, nominal rate stated) and, measured in the same process, the
    FULL MSR3D step at 4 x 576 tokens with e4m3 and with bf16 projections as extra.full_step."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "16", "--warmup", "2",
                          "--cpu-baseline-seconds", "1", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    r = j["roofline"]
    assert set(r["levels"]) == {"level1", "level2", "level3"} and 0 < r["frac"] < 1
    # the line's kernel is the LONGEST launch of the step (census after the timed region), every launch >= 15 us beside it
    longest = max(r["kernels"].values(), key=lambda k: k["us"])
    assert r["kernel"].startswith(longest["kernel"]) and abs(r["kernel_ms"] * 1e3 - longest["us"]) < 0.1
    assert len(r["kernels"]) >= 10 and all(k["us"] >= 15 for k in r["kernels"].values()) and "census" in r["timed"]
    for key in ("msr3d_scene_block[attn_fwd]", "msr3d_scene_block[attn_bwd]", "msr3d_scene_block[ffn_fwd]"):
        assert 0 < r["kernels"][key]["frac"] < 1 and r["kernels"][key]["launches_per_step"] == 3.0
    assert j["config"]["encoder_prefetch"] is True
    ex = j["extra"]
    assert ex["dense_neighbourhoods"]["ms_per_step"] > j["ms_per_step"]                   # the distinct-row kernels' worst case
    assert ex["dense_neighbourhoods"]["distinct_rows_per_launch"]["level2"] == ex["dense_neighbourhoods"]["nominal_rows_per_launch"]["level2"]
    assert ex["as_object"]["value"] > 0 and ex["no_pipeline"]["value"] > 0
    assert ex["bf16_trainable"]["ms_per_step"] < ex["no_pipeline"]["ms_per_step"]
    assert 1e-4 < ex["bf16_trainable"]["rel_l2_vs_f32"]["scene_embeds"] < 2e-2
    assert set(ex["object_attention"]) >= {"attn_fwd", "attn_bwd"}
    for lv in r["levels"].values():
        assert 0 < lv["frac"] < 1 and lv["distinct_rows"] <= lv["nominal_rows"] and lv["kernel_ms"] > 0
    assert r["levels"]["level2"]["distinct_rows"] < 0.2 * r["levels"]["level2"]["nominal_rows"]      # ~9 % on these scenes
    fs = j["extra"]["full_step"]
    for k in ("fp8", "bf16"):
        assert fs[k]["value"] > 0 and fs[k]["config"]["layers"] == 32 and fs[k]["config"]["tokens_per_sequence"] == 576, fs
    assert fs["fp8"]["ms_per_step"] < fs["bf16"]["ms_per_step"]


@pytest.mark.parametrize("extra", [[], ["--unfrozen", "--batch", "2"]])
def test_bench_exchange_captured_inside_the_step_graph(extra):
    """MSR3D_DP_GRAPH_COMM=1: the RCCL call is captured with forward, backward and the optimiser -- one graph
    per step at N > 1, no next batch needed; unfrozen backbone: buckets leave from the backward hooks (forks of
    the capture onto the communication stream)."""
    # (a port of its own per case: the previous case's listener may still be in TIME_WAIT)
    env = dict(os.environ, MSR3D_BENCH_FORCE_DIST="1", MSR3D_DP_GRAPH_COMM="1", MASTER_PORT=str(29674 + 2 * len(extra)),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    # (Round 4 retried this case on hipErrorCapturedEvent, "one unfrozen run in four": buckets that complete inside
    # backward hooks -- autograd worker threads -- during the capture are now left to the capturing thread, dp.py::_launch.
    # No retry.)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2",
                          "--no-cpu-baseline"] + extra, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["config"]["exchange_inside_graph"] is True and j["config"]["hip_graph"] is True
    assert j["config"]["allreduce_hidden_behind_next_encoder"] is False
    assert j["comm"]["ranks_seen"] == 1 and j["comm"]["replica_checksum_spread"] == 0.0 and j["value"] > 0


def test_bench_default_multi_rank_schedule_is_the_captured_exchange_after_its_self_check():
    """World > 1 on RCCL with MSR3D_DP_GRAPH_COMM unset (what an 8-GPU driver run takes): the exchange is captured in the
    step's graph after the start-up self-check -- two replays against two eager steps from the same state -- and the line
    says so; no retry."""
    env = dict(os.environ, MSR3D_BENCH_FORCE_DIST="1", MASTER_PORT="29679", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MSR3D_DP_GRAPH_COMM"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2",
                          "--no-cpu-baseline"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["config"]["exchange_inside_graph"] is True, out.stderr[-2000:]
    chk = j["comm"]["graph_comm_check"]
    assert chk["captured"] is True and chk["replica_checksum_spread"] == 0.0
    assert chk["max_abs_diff"] <= 2.0 * chk["eager_moved"] + 1e-6 * chk["scale"] and chk["eager_moved"] > 0
    assert j["comm"]["ranks_seen"] == 1 and j["comm"]["replica_checksum_spread"] == 0.0 and j["value"] > 0


def test_bench_llm_stack_line():
    """The language-model side of a step as a labelled secondary line: layers + head + loss + exchange + optimiser."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--llm-stack", "1", "--steps", "2", "--warmup", "1"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["metric"].startswith("SECONDARY") and j["unit"] == "tokens/s" and j["value"] > 0
    assert j["config"]["layers"] == 1 and j["config"]["lora_parameters"] == 4 * 131072 + 3 * 241664


def test_bench_plain_python_launches_its_own_ranks():
    """`python bench.py --gpus 2` WITHOUT a launcher (how the driver's N = 1 record invokes it): the script re-executes
    itself under torch.distributed.run and rank 0 still prints exactly one JSON line of a 2-rank run."""
    env = dict(os.environ, MSR3D_BENCH_SINGLE_DEVICE="1", MSR3D_BENCH_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                          "--batch", "4"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["comm"]["ranks_seen"] == 2 and j["comm"]["replica_checksum_spread"] == 0.0
    assert j["config"]["global_batch"] == 8 and j["value"] > 0


def test_bench_full_step_line():
    """The full MSR3D step (hot path joined to the LoRA-Llama stack) as a labelled secondary line; 2 layers here, the
    one-rank RCCL communicator so that the bucketed exchange from the backward hooks really runs."""
    env = dict(os.environ, MSR3D_BENCH_FORCE_DIST="1", MASTER_PORT="29691", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full-step", "--llm-layers", "2", "--steps", "2",
                          "--warmup", "1", "--batch", "2", "--seq-len", "256"], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["metric"].startswith("SECONDARY") and j["unit"] == "samples/s" and j["value"] > 0
    c = j["config"]
    assert c["layers"] == 2 and c["sequences_per_gpu"] == 2 and c["prompter_schedule"] == "blocks"
    assert c["lora_parameters"] == 2 * (4 * 131072 + 3 * 241664) and c["grad_bytes"] > 4 * c["lora_parameters"]
    assert j["comm"]["ranks_seen"] == 1 and j["comm"]["collectives_per_step"] >= 2
    assert j["comm"]["replica_checksum_spread"] == 0.0 and j["comm"]["exchange_exposed_ms_per_step"] >= 0


def _plain_run(out_dir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                          "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_only_and_dumps_the_last_step(tmp_path):
    """A plain run reports the timed steps and nothing that takes runs of its own (census, spread pass, CPU baseline,
    variants); --dump-outputs writes the last timed step's results, and the same arguments give the same inputs."""
    import numpy as np
    runs = [_plain_run(tmp_path / f"run{i}") for i in range(2)]
    j = runs[0]
    assert j["steps"] == 3 and j["warmup"] == 2 and j["value"] > 0 and j["ms_per_step"] > 0
    assert abs(j["value"] - 16 * 1e3 / j["ms_per_step"]) < 1e-6 * j["value"]
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in j, k
    for k in ("roofline", "census_us", "cpu_baseline", "extra", "ms_per_step_percentiles", "kernels_ms"):
        assert k not in j, k
    arrays = [{n: np.load(tmp_path / f"run{i}" / f"{n}.npy") for n in ("loss", "scene_embeds", "obj_embeds", "params")}
              for i in range(2)]
    a = arrays[0]
    assert set(j["dumped_outputs"]["arrays"]) == set(a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["scene_embeds"].shape == (16, 60, 4096) and a["obj_embeds"].shape == (16, 60, 768)
    for n, x in a.items():
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        y = arrays[1][n].astype(np.float64)
        assert np.linalg.norm(x - y) <= 1e-5 * max(np.linalg.norm(y), 1e-30), n     # same inputs, same results
