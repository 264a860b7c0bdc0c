"""bench.py command-line contract: result line fields and --dump-outputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_make_clip_matches_definition():
    """The clip is (position + frame shift + seeded texture) mod 256 per
    channel, including shifts that wrap past 256."""
    n, h, w = 131, 33, 47
    got = _load_bench().make_clip(n, h=h, w=w)
    yy, xx = np.mgrid[0:h, 0:w]
    tex = np.random.RandomState(0).randint(0, 32, size=(h, w, 3))
    for i in (0, 1, 85, 86, 128, 130):
        want = np.stack([xx + 2 * i + tex[:, :, 0], yy + i + tex[:, :, 1],
                         xx + yy + 3 * i + tex[:, :, 2]], axis=-1) % 256
        np.testing.assert_array_equal(got[i], want)
    assert got.dtype == np.uint8 and got.shape == (n, h, w, 3)


def test_bench_dump_outputs(tmp_path):
    """A tiny hist run writes the last timed step's histogram column as
    float64 rows that match the deterministic input clip exactly."""
    n, steps = 8, 2
    dump = tmp_path / "dump"
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--pipeline", "hist",
         "--steps", str(steps), "--warmup", "0", "--frames-per-step", str(n),
         "--dump-outputs", str(dump)],
        env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    result = json.loads(r.stdout.strip().splitlines()[-1])
    assert result["steps"] == steps
    assert result["ms_per_step"] > 0
    assert abs(result["value"] - n / (result["ms_per_step"] * 1e-3)) \
        <= 1e-6 * result["value"]

    assert sorted(os.listdir(dump)) == ["histogram.npy"]
    got = np.load(dump / "histogram.npy")
    assert got.dtype == np.float64 and got.shape == (n, 3 * 256)

    clip = _load_bench().make_clip(n)
    expect = np.stack([
        np.concatenate([np.bincount(f[:, :, c].ravel(), minlength=256)
                        for c in range(3)]) for f in clip])
    np.testing.assert_array_equal(got, expect)
