"""bench.py as later measurements call it: a plain run (`--gpus 1 --steps K --warmup W`) prints one JSON line with the
headline figures only and `ms_per_step`; `--dump-outputs DIR` writes what the last timed step returned (codes and PCM
of every utterance) as float32 .npy files.  Run on the tiny preset so the whole process takes a few seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("batch1", "first_packet_p50_ms", "first_packet_p50_ms_b1", "roofline", "frame_roofline", "kernel_table",
             "gateup_roofline", "prefill_mfma", "cpu_baseline")


def test_plain_run_dumps_last_step_outputs(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, frames = 2, 6
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "QT_BENCH_DRYRUN")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--preset", "tiny-customvoice", "--batch", str(B), "--frames", str(frames),
                        "--prompt-tokens", "12", "--dump-outputs", str(tmp_path / "out")],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["n_gpus"] == 1 and j["full"] is False
    assert j["unit"] == "audio-seconds/sec" and j["higher_is_better"] is True and j["dtype"] == "bf16"
    assert j["ms_per_step"] > 0
    # value = audio seconds of the timed steps / their wall time; a frame is at most 1920 samples of 24 kHz PCM (the
    # codec trims a fixed tail), so value x seconds per step is at most B x frames x 1920 / 24000 (+ rounding)
    assert 0 < j["value"] * j["ms_per_step"] * 1e-3 <= B * frames * 1920 / 24000.0 * 1.01
    assert not [k for k in FULL_ONLY if k in j], "a plain run measures the headline figures only"
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted([f"codes_{i}.npy" for i in range(B)] + [f"pcm_{i}.npy" for i in range(B)])
    for i in range(B):
        codes = np.load(tmp_path / "out" / f"codes_{i}.npy")
        pcm = np.load(tmp_path / "out" / f"pcm_{i}.npy")
        assert codes.dtype == np.float32 and pcm.dtype == np.float32
        assert codes.ndim == 2 and codes.shape[0] == frames
        assert np.array_equal(codes, np.round(codes)) and codes.min() >= 0
        assert pcm.ndim == 1 and (frames - 1) * 1920 - 555 < pcm.shape[0] <= frames * 1920  # 555: the codec's trim
        assert np.isfinite(pcm).all() and np.abs(pcm).max() > 0
