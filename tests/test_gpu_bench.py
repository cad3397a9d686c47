"""bench.py without --full, as a fresh process: the headline line alone on stdout, no extras file, no record on stderr,
and the --dump-outputs arrays -- on one GPU and with two ranks sharing it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("stages_ms", "dispersion", "device", "graph_replay", "cpu_baseline", "cpu_baseline_sampler", "sampler", "gather",
             "pubmed_scale_step", "bgp_scale_step", "collectives", "bgp_strong", "configs4_replicated", "configs4_sharded",
             "extras")


@pytest.mark.parametrize("gpus", [1, 2])
def test_plain_run_prints_the_headline_alone(gpus, tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PN_BENCH_EXTRAS=str(tmp_path / "extras.json"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "PN_DIST_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "4", "--warmup", "2"]
    if gpus == 1:
        cmd += ["--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]       # (gloo prints lines of its own with two ranks)
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1500:], r.stderr[-3000:])
    assert '"metric"' not in r.stderr and not (tmp_path / "extras.json").exists()
    line = json.loads(lines[0])
    assert line["metric"] == "paths aggregated/sec (PAGG fwd+bwd, one training step incl. on-GPU MERW sampling + Adam)"
    assert line["unit"] == "paths/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["n_gpus"] == gpus and line["steps"] == 4 and line["warmup"] == 2 and line["value"] > 0
    # value = the whole job's paths per step over the mean step time
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / line["config"]["paths_per_step"] - 1.0) < 1e-4
    assert line["roofline"]["kernel"] and not [k for k in FULL_ONLY if k in line]
    if gpus == 1:
        out = tmp_path / "out"
        assert {"loss.npy", "logits.npy", "path_ids.npy", "path_codes.npy"} <= set(os.listdir(out))
        logits = np.load(out / "logits.npy")
        assert logits.dtype == np.float32 and logits.shape[1] == 7 and np.isfinite(logits).all()
