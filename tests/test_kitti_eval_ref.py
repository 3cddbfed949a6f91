"""CPU: the numpy restatement of the KITTI evaluation (tests/ref_kitti_eval.py) against the reference's recorded output
(tests/golden/kitti_eval.npz, written by make_golden_kitti_eval.py). No GPU: cpd_amd.kitti_eval's host code runs with
the restatement's stages in place of the kernels."""
import numpy as np
import pytest

import ref_kitti_eval as R

CLASSES = ["Car", "Pedestrian", "Cyclist"]


@pytest.fixture(scope="module")
def kz(golden):
    return golden("kitti_eval")


@pytest.mark.parametrize("crit", [-1, 0, 1, 2])
def test_rotate_iou_matches_reference(kz, crit):
    want = kz["rot_iou_%s" % ("m1" if crit == -1 else crit)]
    got = R.rotate_iou(kz["rot_boxes"], kz["rot_query"], crit)
    valid = kz["rot_valid"] == 1
    assert valid.mean() > 0.9
    assert np.abs(got[valid] - want[valid]).max() <= 1e-6


def test_official_result_matches_reference(kz):
    gt, dt = R.annos_from_npz(kz, "gt_"), R.annos_from_npz(kz, "dt_")
    assert len(gt) == 100 and any(len(a["name"]) == 0 for a in gt) and any(len(a["name"]) == 0 for a in dt)
    detail = {}
    result, ret = R.get_official_eval_result(gt, dt, CLASSES, PR_detail_dict=detail)
    assert result == str(kz["result"])
    assert list(ret) == list(kz["ret_keys"])
    for k, v in zip(kz["ret_keys"], kz["ret_values"]):
        if "_aos/" in k:
            assert abs(ret[k] - v) <= 1e-9, k
        else:
            assert ret[k] == v, k
    for k in ("bbox", "bev", "3d"):
        np.testing.assert_array_equal(detail[k], kz["pr_" + k])
    np.testing.assert_allclose(detail["aos"], kz["pr_aos"], rtol=0, atol=1e-9)


def test_get_thresholds_matches_serial_scan():
    from cpd_amd.kitti_eval import get_thresholds

    def serial(scores, num_gt):
        # one pass over the scores, high to low: a score becomes a threshold when the recall it gives is at least as
        # close to the next of the 41 sample points as the recall of the score after it, or when it is the last one
        ordered = sorted(np.asarray(scores).tolist(), reverse=True)
        out, target = [], 0
        for rank, value in enumerate(ordered, start=1):
            here = rank / num_gt
            is_last = rank == len(ordered)
            after = here if is_last else (rank + 1) / num_gt
            if is_last or not (after - target < target - here):
                out.append(value)
                target += 1 / 40.0
        return out

    rng = np.random.default_rng(3)
    for n, g in [(0, 5), (1, 1), (7, 40), (300, 310), (1000, 1000), (57, 3)]:
        s = np.round(rng.random(n), 2)
        assert [float(v) for v in get_thresholds(s.copy(), g)] == serial(s, g)
    with pytest.raises(ZeroDivisionError):
        get_thresholds(np.zeros(0), 0)


def test_module_has_no_numba():
    import os
    import cpd_amd
    root = os.path.dirname(cpd_amd.__file__)
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                assert "numba" not in open(os.path.join(dirpath, f)).read(), f
