"""GPU: a plain `bench.py` run is the headline alone, and `--dump-outputs` writes what its last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(cuda, tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["warmup"] == 1 and r["unit"] == "frames/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["ms_per_step"] > 0 and abs(r["value"] - 5 * 1e3 / r["ms_per_step"]) < 1e-6 * r["value"]
    assert not {"roofline", "cpu_baseline", "mask_logit_max_abs_err", "sliding_clip_loop", "config4_swinb_refvos"} & set(r)
    files = sorted(os.listdir(out))
    assert files == ["pred_embds.npy", "pred_logits.npy", "pred_masks_sample.npy"], files
    arrays = {f: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays["pred_logits.npy"].shape == (1, 100, 3938) and arrays["pred_embds.npy"].shape == (1, 100, 5, 256)
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
