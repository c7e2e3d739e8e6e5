"""Driver-contract test: bench.py must run under torch.distributed.run and
print ONE valid JSON line with the agreed keys, for the parallel layouts the
driver launches (dp2 at N=2; dp2*pp2*tp2 at N=8).

These are contract tests, not multi-GPU coverage: on a machine with fewer
GPUs than ranks (a CPU-only or a one-GPU box) the launched ranks run on
gloo/CPU and never touch the GPU or RCCL.  Only with at least as many GPUs
as ranks do the multi-rank layouts exercise the GPU path."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}
# hides every GPU from a child process (an empty value does not)
_NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}


def _run_bench(nproc, port, extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(REPO, "bench.py"),
           "--gpus", str(nproc), "--steps", "2", "--warmup", "1"] + extra
    env = dict(os.environ)
    import torch
    if 0 < torch.cuda.device_count() < nproc:
        # RCCL refuses two ranks on one device: with fewer GPUs than ranks
        # the contract is checked on the gloo/CPU path, as on a CPU-only box
        env.update(_NO_GPU)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                         cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE json line, got: {out.stdout[-500:]}"
    payload = json.loads(lines[0])
    assert REQUIRED <= set(payload), REQUIRED - set(payload)
    assert payload["n_gpus"] == nproc
    assert payload["value"] > 0 and payload["ms_per_step"] > 0
    return payload


def test_bench_json_contract_dp2():
    p = _run_bench(2, 29601, ["--model", "tiny", "--batch", "2"])
    assert p["config"]["parallelism"] == "dp2_pp1_tp1"


def _run_plain(extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
           "--model", "tiny", "--batch", "2", "--seq", "32"] + extra
    # single-process CPU run regardless of the box the suite runs on
    env = dict(os.environ, **_NO_GPU)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                         cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE json line, got: {out.stdout[-500:]}"
    return json.loads(lines[0])


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float32 .npy,
    identical between two runs with the same arguments (seeded inputs), and
    --steps sets the number of optimizer steps they went through."""
    import numpy as np
    dumps = {}
    for tag, steps in (("a", 2), ("b", 2), ("c", 3)):
        d = tmp_path / tag
        p = _run_plain(["--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(d)])
        assert REQUIRED <= set(p) and p["steps"] == steps
        assert p["ms_per_step"] > 0
        dumps[tag] = {f: np.load(d / f) for f in sorted(os.listdir(d))}
    a, b, c = dumps["a"], dumps["b"], dumps["c"]
    assert set(a) == {"loss.npy", "logits.npy", "params.npy"}
    total = 0
    for name, arr in a.items():
        assert arr.dtype == np.float32 and np.isfinite(arr).all(), name
        total += arr.nbytes
        np.testing.assert_array_equal(arr, b[name])
    assert total <= 64 << 20
    assert a["loss.npy"].shape == (1,)
    assert a["logits.npy"].shape == (2, 32, 2048)
    # one more timed step = one more AdamW update: the outputs must move
    assert not np.array_equal(a["params.npy"], c["params.npy"])
    assert c["loss.npy"][0] < a["loss.npy"][0]


@pytest.mark.gpu
def test_bench_dump_outputs_graph_path_gpu(tmp_path):
    """tiny defaults to the hipGraph-captured step on a GPU: the dump then
    holds the loss and the parameter sample (the logits stay inside the
    graph's memory pool), read after the LAST replay: one more timed replay
    must move both (a value left from capture or warmup would not)."""
    import numpy as np
    dumps = {}
    for steps in (2, 3):
        d = tmp_path / f"s{steps}"
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
               "--model", "tiny", "--batch", "2", "--seq", "64",
               "--steps", str(steps), "--warmup", "1",
               "--dump-outputs", str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True,
                             timeout=300, cwd=REPO)
        assert out.returncode == 0, out.stderr[-2000:]
        p = json.loads([ln for ln in out.stdout.splitlines()
                        if ln.startswith("{")][0])
        assert p["dtype"] == "bf16" and p["steps"] == steps
        assert sorted(os.listdir(d)) == ["loss.npy", "params.npy"]
        loss = np.load(d / "loss.npy")
        params = np.load(d / "params.npy")
        assert loss.dtype == np.float32 and loss.shape == (1,)
        # a small-init 2048-way classifier starts near ln(2048) = 7.6 and a
        # few AdamW steps on one batch only lower that: above is garbage
        assert 0.0 < loss[0] < 7.62 + 1.0
        assert params.dtype == np.float32 and np.isfinite(params).all()
        assert params.size > 10000 and np.abs(params).max() > 0
        dumps[steps] = (loss, params)
    assert dumps[2][0][0] != dumps[3][0][0]
    assert not np.array_equal(dumps[2][1], dumps[3][1])


def test_bench_full_flag_plain_layout():
    """--full is accepted, and on a layout with nothing extra to measure it
    leaves the result line's keys as a plain run's.  This does NOT verify
    the gate itself: that a plain dp>1 GPT-2 GPU run leaves
    ``torchddp_ms_per_step`` out and ``--full`` puts it in needs at least
    two GPUs and is covered by no test."""
    p = _run_plain(["--steps", "1", "--warmup", "0", "--full"])
    assert REQUIRED <= set(p)
    assert "torchddp_ms_per_step" not in p["config"]


@pytest.mark.slow
def test_bench_json_contract_8rank(tmp_path):
    import numpy as np
    p = _run_bench(8, 29602, ["--model", "tiny", "--batch", "2",
                              "--dump-outputs", str(tmp_path)])
    assert p["config"]["parallelism"] == "dp2_pp2_tp2"
    # pipeline --dump-outputs: every rank writes its stage's parameter
    # sample, the last-stage ranks also their loss.  Axes are ordered
    # [data, pipe, tensor] with tensor innermost: rank = d*4 + p*2 + t
    last_stage = {r for r in range(8) if (r // 2) % 2 == 1}
    want = {f"params_rank{r}.npy" for r in range(8)} | \
        {f"loss_rank{r}.npy" for r in last_stage}
    assert set(os.listdir(tmp_path)) == want
    for f in want:
        arr = np.load(tmp_path / f)
        assert arr.dtype == np.float32 and arr.size > 0, f
        assert np.isfinite(arr).all(), f


@pytest.mark.slow
def test_bench_json_contract_zero_tp():
    """ZeRO + TP composition through the real bench flow (the r01-advisor
    bug class: SP grads must survive ZeRO's bucketing)."""
    os.environ["TDPA_PARALLEL"] = "2,1,2"
    try:
        p = _run_bench(4, 29603, ["--model", "tiny", "--batch", "4",
                                  "--zero"])
    finally:
        os.environ.pop("TDPA_PARALLEL", None)
    assert p["config"]["parallelism"] == "dp2_pp1_tp2"
