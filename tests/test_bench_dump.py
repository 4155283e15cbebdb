"""CPU: bench.py --dump-outputs writes float32 / float64 arrays under the 64 MB cap, the full outputs when they fit and the same seeded
pixel sample from run to run when they do not, with whole-output sums beside the sample."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def outputs(F, H, W, max_inst, seed):
    rng = np.random.default_rng(seed)
    a = {"frames": rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8), "instance_counts": rng.integers(0, max_inst + 1, F)}
    if max_inst:
        a["masks"] = rng.random((F, max_inst, H, W)) < 0.3
    return a


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    a = outputs(2, 48, 40, 2, 0)
    shapes = bench.dump_outputs(a, str(tmp_path))
    got = load(str(tmp_path))
    assert set(got) == set(shapes) == {"frames", "masks", "instance_counts", "frame_channel_sums", "mask_areas"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["frames"], a["frames"].astype(np.float32))
    assert np.array_equal(got["masks"], a["masks"].astype(np.float32))
    assert np.array_equal(got["instance_counts"], a["instance_counts"])
    assert np.array_equal(got["mask_areas"], a["masks"].sum((2, 3)))


def test_headline_outputs_are_sampled_under_the_cap(tmp_path):
    """8 frames of 1024 x 1024 with 2 masks each (the default frame workload) are ~160 MB as float32: a fixed pixel sample"""
    a = outputs(8, 1024, 1024, 2, 1)
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    bench.dump_outputs(a, d1)
    bench.dump_outputs(a, d2)
    size = sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1))
    assert size <= 64 << 20
    g1, g2 = load(d1), load(d2)
    assert set(g1) == set(g2) and all(np.array_equal(g1[k], g2[k]) for k in g1)
    idx = g1["pixel_index"].astype(np.int64)
    assert len(idx) > 100000 and len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < 1024 * 1024
    assert np.array_equal(g1["frames"], a["frames"].reshape(8, -1, 3)[:, idx].astype(np.float32))
    assert np.array_equal(g1["masks"], a["masks"].reshape(8, 2, -1)[:, :, idx].astype(np.float32))
    assert np.array_equal(g1["frame_channel_sums"], a["frames"].reshape(8, -1, 3).sum(1, dtype=np.float64))


def test_frames_only_outputs(tmp_path):
    """the warp workload: one 1024 x 1024 frame, no masks, written whole"""
    a = {"frames": outputs(1, 1024, 1024, 0, 2)["frames"]}
    shapes = bench.dump_outputs(a, str(tmp_path))
    assert shapes == {"frames": [1, 1024, 1024, 3], "frame_channel_sums": [1, 3]}
