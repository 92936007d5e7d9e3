"""``bench.py`` on one GPU with a shrunk GPT-J: a plain run measures the headline only,
``--dump-outputs`` writes what the last timed step computed, and the same arguments give the same outputs."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--layers", "2", "--hidden", "1024", "--heads", "4", "--seq", "512", "--micro-batch", "2", "--gas", "2",
           "--tunableop", "off", "--dump-outputs", out_dir]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


def _load(d):
    return np.load(os.path.join(d, "loss.npy")), np.load(os.path.join(d, "params_sample.npy"))


@pytest.fixture(scope="module")
def first(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump_a"))
    return (d,) + _run(d)


def test_plain_run_is_headline_only_and_dumps_outputs(first):
    d, rec, err = first
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["dtype"] == "bf16" and rec["higher_is_better"] is True and rec["unit"] == "tokens/s"
    # tokens/s and ms_per_step describe the same timed steps (global batch 4 x 512 tokens)
    assert rec["value"] == pytest.approx(4 * 512 / (rec["ms_per_step"] / 1e3), rel=1e-2)
    assert rec["secondary"] is None and not [k for k in rec if k.startswith("secondary_") or k == "bloom_tp"]
    assert sorted(os.listdir(d)) == ["loss.npy", "params_sample.npy"]
    loss, params = _load(d)
    assert loss.dtype == np.float32 and loss.shape == (1,) and np.isfinite(loss).all() and 0 < loss[0] < 12
    assert params.dtype == np.float32 and params.ndim == 1 and np.isfinite(params).all() and params.std() > 0
    assert loss.nbytes + params.nbytes < 64 * 2**20
    # the dumped loss is the last timed step's: the value the run reports with four decimals
    reported = float(re.search(r"^\[bench\] loss=([0-9.]+) ", err, re.M).group(1))
    assert abs(float(loss[0]) - reported) < 1e-4


def test_same_arguments_give_the_same_outputs(first, tmp_path):
    """Model, token ids and sample positions are seeded and the one-GPU step sums in a fixed order,
    so a second run writes the same bytes: what lets two builds be compared output for output."""
    loss_a, params_a = _load(first[0])
    _run(str(tmp_path))
    loss_b, params_b = _load(str(tmp_path))
    assert np.array_equal(loss_a, loss_b), (loss_a, loss_b)
    assert params_a.shape == params_b.shape
    assert np.array_equal(params_a, params_b), float(np.abs(params_a - params_b).max())
