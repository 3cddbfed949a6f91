"""bench.py --dump-outputs on the CPU: the files a caller of the timed path is compared by (float32 .npy, at most 64 MB in all,
the same rows in every run, boxes and scores kept paired)."""
import os

import numpy as np
import torch

import bench


def _dump(d, arrays):
    bench.dump_outputs(str(d), arrays)
    return {f[:-4]: np.load(os.path.join(str(d), f)) for f in sorted(os.listdir(str(d)))}


def test_detection_arrays_concatenate_frames_in_order():
    res = [{"pred_boxes": torch.arange(21, dtype=torch.float32).reshape(3, 7), "pred_scores": torch.tensor([0.9, 0.5, 0.1]),
            "pred_labels": torch.tensor([1, 2, 3])},
           {"pred_boxes": torch.zeros((0, 7)), "pred_scores": torch.zeros(0), "pred_labels": torch.zeros(0, dtype=torch.int64)},
           {"pred_boxes": torch.full((1, 7), 5.0), "pred_scores": torch.tensor([0.7]), "pred_labels": torch.tensor([1])}]
    a = bench.detection_arrays(res)
    assert sorted(a) == ["boxes_per_frame", "pred_boxes", "pred_labels", "pred_scores"]
    np.testing.assert_array_equal(a["boxes_per_frame"], [3, 0, 1])
    np.testing.assert_array_equal(a["pred_boxes"], np.concatenate([np.arange(21).reshape(3, 7), np.full((1, 7), 5.0)]))
    np.testing.assert_array_equal(a["pred_scores"], np.float32([0.9, 0.5, 0.1, 0.7]))
    np.testing.assert_array_equal(a["pred_labels"], [1, 2, 3, 1])


def test_small_outputs_are_written_whole_as_float32(tmp_path):
    arrays = {"pred_boxes": np.arange(70, dtype=np.float64).reshape(10, 7), "pred_labels": np.arange(10, dtype=np.int64),
              "loss": np.float64(0.25)}
    got = _dump(tmp_path, arrays)
    assert sorted(got) == ["loss", "pred_boxes", "pred_labels"]
    for k, v in arrays.items():
        assert got[k].dtype == np.float32
        np.testing.assert_array_equal(got[k], np.asarray(v, np.float32).reshape(got[k].shape))
    assert got["pred_boxes"].shape == (10, 7) and got["loss"].shape == (1,)


def test_large_outputs_keep_a_fixed_paired_sample_within_64_mb(tmp_path):
    n = 3_000_000                                              # 84 MB of boxes + 12 MB of scores + 12 MB of labels
    ids = np.arange(n, dtype=np.float32)
    boxes = np.repeat(ids[:, None], 7, 1)
    arrays = {"pred_boxes": boxes, "pred_scores": ids, "pred_labels": ids, "boxes_per_frame": np.array([n]), "loss": np.float32(1.5)}
    a = _dump(tmp_path / "a", arrays)
    b = _dump(tmp_path / "b", arrays)
    on_disk = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert on_disk <= 64 * 10 ** 6
    assert on_disk > 60 * 10 ** 6                              # a sample, not a handful of rows
    for k in arrays:
        assert a[k].tobytes() == b[k].tobytes()                # the same rows in every run
    rows = a["pred_scores"]
    assert 0 < rows.shape[0] < n and np.all(np.diff(rows) > 0)    # distinct rows, in their original order
    np.testing.assert_array_equal(a["pred_boxes"], np.repeat(rows[:, None], 7, 1))   # each kept box with its own score
    np.testing.assert_array_equal(a["pred_labels"], rows)
    np.testing.assert_array_equal(a["boxes_per_frame"], [n])   # single-row outputs are kept whole
    assert a["loss"].tolist() == [1.5]                     # a scalar is written as one element
