"""bench.py --dump-outputs: the frame the last timed step computed, written as float64 .npy so that two builds can be compared
output for output.  The writer itself runs without a GPU; the -m gpu test checks that what bench.py writes is the timed frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import functracer_amd as ft

from . import helpers as H

sys.path.insert(0, H.ROOT)
import bench  # noqa: E402


def test_dump_budget_covers_the_headline_frame_and_bounds_the_sample():
    assert 1920 * 1080 * 3 * 8 <= bench.DUMP_MAX_BYTES                       # the headline frame is written whole
    assert 3840 * 2160 * 3 * 8 > bench.DUMP_MAX_BYTES                        # config 5's frame is sampled
    assert bench.DUMP_SAMPLE_PIXELS * (3 + 1) * 8 + 2 * 4096 <= bench.DUMP_MAX_BYTES   # sample + index + two .npy headers


def test_dump_writes_a_frame_that_fits_whole(tmp_path):
    frame = np.random.default_rng(1).normal(size=(54, 96, 3))
    info = bench.dump_outputs(str(tmp_path), frame)
    got = np.load(tmp_path / "frame.npy")
    assert got.dtype == np.float64 and np.array_equal(got, frame)
    assert info["files"] == {"frame.npy": [54, 96, 3]} and sorted(os.listdir(tmp_path)) == ["frame.npy"]


def test_dump_samples_a_large_frame_with_a_fixed_seed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 54 * 96 * 3 * 8 - 1)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_PIXELS", 500)
    bench.dump_outputs(str(tmp_path), np.zeros((2, 2, 3)))                   # an earlier, smaller frame: its frame.npy must go
    frame = np.random.default_rng(2).normal(size=(54, 96, 3))
    info = bench.dump_outputs(str(tmp_path), frame)
    assert sorted(os.listdir(tmp_path)) == ["frame_sample.npy", "frame_sample_index.npy"]
    assert info["files"] == {"frame_sample.npy": [500, 3], "frame_sample_index.npy": [500]}
    sample, index = np.load(tmp_path / "frame_sample.npy"), np.load(tmp_path / "frame_sample_index.npy")
    assert sample.dtype == np.float64 and index.dtype == np.float64
    assert (np.diff(index) > 0).all() and index[0] >= 0 and index[-1] < 54 * 96
    assert np.array_equal(sample, frame.reshape(-1, 3)[index.astype(np.int64)])
    bench.dump_outputs(str(tmp_path), frame)                                 # same frame, same sample
    assert np.array_equal(np.load(tmp_path / "frame_sample_index.npy"), index)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_dump_is_the_frame_the_timed_steps_rendered(tmp_path, hip):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(H.ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--side-steps", "0", "--no-cpu-baseline",
           "--no-alone", "--no-boundary", "--prewarm-ms", "0", "--dump-outputs", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=500, cwd=H.ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    d = json.loads([line for line in res.stdout.splitlines() if line.startswith("{")][0])
    assert d["steps"] == 3 and d["workloads"]["headline"]["steps"] == 3 and d["ms_per_step"] > 0
    assert d["dump_outputs"]["files"] == {"frame.npy": [1080, 1920, 3]}
    got = np.load(out / "frame.npy")
    p = ft.parse_scene_file(H.scene_path("bunny"))
    p.lower(hip)
    want, _ = hip.render(p.camera, 1920, 1080, 16, ft.jitter_pattern(16))
    assert got.dtype == np.float64 and np.array_equal(got, want)
