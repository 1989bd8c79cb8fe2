"""GPU tests of bench.py's plain run (the headline line and nothing else) and of --dump-outputs: what the timed path
returned in its last step, written as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cold_start", "parity", "without_gather", "exact_fp32", "roofline", "roofline_hbm_stage",
             "host_enqueue_ms_per_forward", "range_guard", "host_to_host", "cpu_baseline", "other_configs",
             "strong_scaling_job", "summary")


def _plain(*args, **env):
    e = dict(os.environ, **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "FV_BENCH_FORCE_DIST"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bench.py"), "--gpus", "1", *args], env=e,
                       cwd=cases.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_timed_output(tmp_path, golden_dir):
    """A plain run prints the headline fields and none of --full's legs; the dumped waveform is the reference's output
    for utterance 0 (the parity check a --full run makes inside bench.py)."""
    out = _plain("--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert all(k in out for k in HEADLINE) and out["higher_is_better"] is True and out["unit"] == "samples/s"
    assert not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == 4 and out["warmup"] == 1
    assert abs(out["value"] - 240000 * 4 / (out["ms_per_step"] * 4e-3)) / out["value"] < 1e-6
    assert sorted(os.listdir(tmp_path)) == ["wav.npy"]
    wav = np.load(tmp_path / "wav.npy")
    assert wav.dtype == np.float32 and wav.shape == (1, 240000) and np.isfinite(wav).all()
    g = np.load(os.path.join(golden_dir, "full_hifigan_light.npz"))
    assert wav.size == int(g["T1000_n"])
    assert float(np.abs(wav[0][g["T1000_idx"]].astype(np.float64) - g["T1000_samples"]).max()) <= 1e-4


def test_plain_job_run_dumps_the_int16_waveforms(tmp_path):
    """--config large512 (shrunk to 6 utterances): the job's int16 rows as float32, every row, in utterance order."""
    out = _plain("--config", "large512", "--steps", "1", "--warmup", "0", "--sub", "4", "--dump-outputs", str(tmp_path),
                 FV_BENCH_JOB="6")
    assert out["scaling"] == "strong" and out["config"]["global_batch"] == 6 and out["steps"] == 1
    assert sorted(os.listdir(tmp_path)) == ["pcm.npy"]
    pcm = np.load(tmp_path / "pcm.npy")
    assert pcm.dtype == np.float32 and pcm.shape == (6, 240000)
    assert np.array_equal(pcm, np.round(pcm)) and np.abs(pcm).max() <= 32767
    assert (np.abs(pcm).max(axis=1) > 0).all() and not np.array_equal(pcm[0], pcm[1])   # six different utterances
