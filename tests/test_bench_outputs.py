"""bench.py's plain run and --dump-outputs: a plain run prints the headline line alone (nothing
that --full adds), and the frame it dumps is, bit for bit, the library's render of the same
configuration; frames over the size limit are cut to a fixed, seeded sample of their rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("frame_wall_ms", "frame_latency_ms", "roofline", "parity", "corrected_camera", "cpu_baseline",
             "dropin_first_ms", "segments_per_primary")


def test_dump_outputs_samples_large_frames(tmp_path):
    import bench
    small = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    bench.dump_outputs(str(tmp_path / "s"), small)
    got = np.load(tmp_path / "s" / "frame.npy")
    assert got.dtype == np.float32 and not (tmp_path / "s" / "frame_rows.npy").exists()
    np.testing.assert_array_equal(got, small.astype(np.float32))
    H, W = 1500, 4096  # 70.3 MiB in f32: over the limit
    big = np.arange(H, dtype=np.float32)[:, None, None] + np.zeros((1, W, 3), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    rows = np.load(tmp_path / "a" / "frame_rows.npy")
    frame = np.load(tmp_path / "a" / "frame.npy")
    assert rows.dtype == np.float64 and frame.dtype == np.float32
    assert len(rows) == len(frame) < H and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(frame[:, 0, 0], rows)  # row i of the sample is row rows[i] of the frame
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT and total > bench.DUMP_LIMIT - 2 * big[0].nbytes
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "frame_rows.npy"))  # the same sample every run


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_frame(tmp_path):
    """Config 1 (simple scene, 200x100 @1 spp): the dumped frame equals rt.render_f32's."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "c1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(k in rec for k in HEADLINE) and not any(k in rec for k in FULL_ONLY)
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["frames_issued"] == 4
    assert rec["ms_per_step"] > 0 and rec["unit"] == "Mrays/s"
    # value is the primary rays of the timed steps over their time; both are printed to 3 decimals
    assert rec["value"] == pytest.approx(200 * 100 * 1 / (rec["ms_per_step"] * 1e-3) / 1e6,
                                         rel=0.0005 / rec["ms_per_step"] + 1e-3)
    assert sorted(os.listdir(out)) == ["frame.npy"]
    frame = np.load(out / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (100, 200, 3)
    import raytracinginoneweekend_amd as rt
    ref, _ = rt.render_f32(rt.simple_scene_arrays(), rt.make_params(200, 100, 1, 64, 1234))
    np.testing.assert_array_equal(frame.view(np.uint32), np.asarray(ref).reshape(100, 200, 3).view(np.uint32))
