"""bench.py's plain run and ``--dump-outputs``: the result line holds the headline fields and nothing that needs
runs of its own (those come with ``--full``), ``--steps`` sets the number of timed steps, and the dumped frame is
the frame a single device renders for the last timed view."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    # bench.py sets the HIP queue count for its own process at import; this one keeps what it had
    queues = os.environ.get("GPU_MAX_HW_QUEUES")
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    if queues is None:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    return bench


def test_dump_of_a_large_frame_is_a_fixed_sample_within_the_budget(tmp_path):
    import torch
    bench = _bench()
    frame = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2160, 3840, 3), dtype=np.uint8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame)
    assert sorted(os.listdir(tmp_path / "a")) == ["frame_sample.npy", "frame_sample_pixels.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
    sample, pixels = (np.load(tmp_path / "a" / f) for f in ("frame_sample.npy", "frame_sample_pixels.npy"))
    assert sample.dtype == np.float32 and pixels.dtype == np.float64
    assert np.array_equal(sample, frame.numpy().reshape(-1, 3)[pixels.astype(np.int64)])
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


@pytest.mark.gpu
def test_plain_run_and_dumped_frame(api, tmp_path):
    import scenes
    steps, warmup, fps = 3, 1, 16
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--frames-per-step", str(fps), "--dump-outputs", str(out_dir)]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["steps"] == steps and line["config"]["frames_per_step"] == fps
    assert line["config"]["timed_frames"] == steps * fps
    assert not {"cpu_baseline", "roofline", "latency_ms_single", "scene_render_ms_host"} & set(line)

    assert os.listdir(out_dir) == ["frame.npy"]
    frame = np.load(out_dir / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (1080, 1920, 3)
    # every frame of the warm-up and of the timed steps is one of N_VIEWS views in turn (fps is a multiple of it)
    bench = _bench()
    scene = scenes.build(api, "c4_torus200k_1080p")
    cam, dbg = bench.swing_cameras(api, scene, bench.N_VIEWS)[((warmup + steps) * fps - 1) % bench.N_VIEWS]
    scene.camera, scene.debug_camera = cam, dbg
    want = scene._backend().render(scene, shadows=True, counters=False)
    assert np.array_equal(frame, want.astype(np.float32))
    scene.close()
