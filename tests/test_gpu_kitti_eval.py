"""GPU: cpd_amd.kitti_eval (csrc/kitti_eval.hip) against the reference's recorded output (tests/golden/kitti_eval.npz)
and, at sizes the reference cannot run in a test, stage by stage against the numpy restatement (tests/ref_kitti_eval.py)."""
import numpy as np
import pytest

import ref_kitti_eval as R

pytestmark = pytest.mark.gpu
CLASSES = ["Car", "Pedestrian", "Cyclist"]


@pytest.fixture(scope="module")
def ke(hip):
    from cpd_amd import kitti_eval
    return kitti_eval


@pytest.fixture(scope="module")
def kz(golden):
    return golden("kitti_eval")


@pytest.fixture(scope="module")
def big():
    return R.synthetic_set(600, seed=11)


@pytest.mark.parametrize("crit", [-1, 0, 1, 2])
def test_rotate_iou_vs_golden(ke, kz, crit):
    want = kz["rot_iou_%s" % ("m1" if crit == -1 else crit)]
    got = ke.rotate_iou_gpu_eval(kz["rot_boxes"], kz["rot_query"], crit)
    assert got.dtype == np.float32 and got.shape == want.shape
    valid = kz["rot_valid"] == 1
    assert np.abs(got[valid] - want[valid]).max() <= 1e-6
    # the pairs the reference's buffer cannot hold still give a finite value here (no write past 8 points)
    assert np.all(np.isfinite(got))


def test_official_result_vs_golden(ke, kz):
    gt, dt = R.annos_from_npz(kz, "gt_"), R.annos_from_npz(kz, "dt_")
    detail = {}
    result, ret = ke.get_official_eval_result(gt, dt, CLASSES, PR_detail_dict=detail)
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


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_stages_vs_numpy_large(ke, big, metric):
    gt, dt = big
    assert len(gt) >= 500
    classes = [0, 1, 2]
    diffs = [0, 1, 2]
    min_overlaps = np.stack([np.array([[0.7, 0.5, 0.5]] * 3), np.array([[0.7, 0.5, 0.5], [0.5, 0.25, 0.25],
                                                                        [0.5, 0.25, 0.25]])], 0)
    frames = ke._Frames(gt, dt, classes, diffs)
    sweeps = ke._sweep_list(3, diffs, min_overlaps, metric)
    run = ke._MetricRun(frames, gt, dt, metric, sweeps)
    ref = R.NumpyRun(frames, gt, dt, metric, sweeps)
    # segmented overlaps, per frame. Image overlaps are float64 and exact. The rotated ones are the reference's float32
    # polygon clipping at coordinates up to 70 m: rounding numpy's float32 sin / cos differently by one ulp alone moves
    # this set's BEV IoUs by up to 1.3e-4 (nearly parallel edges of a detection and its gt), and the device's sinf / cosf
    # are not numpy's -- hence 5e-4 here, and a 1e-3 separation of every overlap from the thresholds in synthetic_set
    tol = 0.0 if metric == 0 else 5e-4
    packed = run.overlaps.cpu().numpy()
    for f, o in enumerate(ref.ovs):
        got = packed[run.pair_off[f]:run.pair_off[f + 1]].reshape(o.shape)
        assert np.abs(got - o).max(initial=0) <= tol, f
    # matching stages on the device's own overlaps, so the comparison is exact
    ref.ovs = [packed[run.pair_off[f]:run.pair_off[f + 1]].reshape(o.shape) for f, o in enumerate(ref.ovs)]
    scores, matched = run.matched_scores()
    rs, rm = ref.matched_scores()
    np.testing.assert_array_equal(matched, rm)
    np.testing.assert_array_equal(scores[matched], rs[rm])
    thresholds = [np.array(ke.get_thresholds(scores[s][matched[s]], int(frames.num_valid_gt[sw[3]])))
                  for s, sw in enumerate(sweeps)]
    compute_aos = metric == 0
    pr = run.pr(thresholds, compute_aos)
    rpr = ref.pr(thresholds, compute_aos)
    np.testing.assert_array_equal(pr[:, :, :3], rpr[:, :, :3])
    np.testing.assert_allclose(pr[:, :, 3], rpr[:, :, 3], rtol=1e-12, atol=1e-9)
    assert pr[:, :, 0].sum() > 1000


def test_whole_set_ap_vs_numpy(ke, big):
    gt, dt = big
    d1, d2 = {}, {}
    res, ret = ke.get_official_eval_result(gt, dt, CLASSES, PR_detail_dict=d1)
    rres, rret = R.get_official_eval_result(gt, dt, CLASSES, PR_detail_dict=d2)
    assert res == rres
    for k in rret:
        assert abs(ret[k] - rret[k]) <= 1e-9 if "_aos/" in k else ret[k] == rret[k], k
    for k in ("bbox", "bev", "3d"):
        np.testing.assert_array_equal(d1[k], d2[k])


def test_edge_cases(ke, kz):
    gt, dt = R.annos_from_npz(kz, "gt_"), R.annos_from_npz(kz, "dt_")
    empty = [{k: v[:0] for k, v in a.items()} for a in dt]
    # no detections anywhere: every AP is 0, like the numpy restatement's
    res, ret = ke.get_official_eval_result(gt, empty, CLASSES)
    rres, rret = R.get_official_eval_result(gt, empty, CLASSES)
    assert res == rres and ret == rret
    assert all(v == 0 for v in ret.values())
    # one frame in all, with gts of every class present somewhere in it
    f = max(range(len(gt)), key=lambda i: len(set(gt[i]["name"]) & {"Car", "Pedestrian", "Cyclist"}) * 100
            + len(dt[i]["name"]))
    cls = sorted(set(gt[f]["name"]) & {"Car", "Pedestrian", "Cyclist"})
    try:
        want = R.get_official_eval_result([gt[f]], [dt[f]], cls)
    except ZeroDivisionError:
        with pytest.raises(ZeroDivisionError):
            ke.get_official_eval_result([gt[f]], [dt[f]], cls)
    else:
        assert ke.get_official_eval_result([gt[f]], [dt[f]], cls) == want
    # a frame whose gts are all DontCare (its detections are suppressed or counted as fp; others unchanged)
    dc = {"name": np.array(["DontCare", "DontCare"]), "truncated": np.array([-1.0, -1.0]), "occluded": np.array([-1, -1]),
          "alpha": np.array([-10.0, -10.0]), "bbox": np.array([[100.0, 150.0, 300.0, 260.0], [700.0, 160.0, 760.0, 200.0]]),
          "dimensions": -np.ones((2, 3)), "location": np.full((2, 3), -1000.0), "rotation_y": np.array([-10.0, -10.0])}
    det = {"name": np.array(["Car", "Pedestrian", "Car"]), "truncated": np.zeros(3), "occluded": np.zeros(3, np.int64),
           "alpha": np.array([0.1, 0.2, 0.3]), "bbox": np.array([[110.0, 155.0, 290.0, 255.0], [705.0, 150.0, 740.0, 200.0],
                                                                  [400.0, 150.0, 480.0, 220.0]]),
           "dimensions": np.array([[3.9, 1.5, 1.6], [0.8, 1.7, 0.6], [3.9, 1.5, 1.6]]),
           "location": np.array([[-5.0, 1.6, 20.0], [3.0, 1.6, 25.0], [0.0, 1.6, 30.0]]), "rotation_y": np.array([0.1, 0.2, 0.3]),
           "score": np.array([0.9, 0.8, 0.7])}
    gt2, dt2 = list(gt) + [dc], list(dt) + [det]
    assert ke.get_official_eval_result(gt2, dt2, CLASSES) == R.get_official_eval_result(gt2, dt2, CLASSES)
    # a class with no valid gt: the reference divides by zero in get_thresholds
    no_cyc = [dict(a, name=np.where(a["name"] == "Cyclist", "Misc", a["name"])) for a in gt]
    with pytest.raises(ZeroDivisionError):
        ke.get_official_eval_result(no_cyc, dt, CLASSES)


def test_repeatable(ke, big):
    gt, dt = big
    d1, d2 = {}, {}
    a = ke.get_official_eval_result(gt, dt, CLASSES, PR_detail_dict=d1)
    b = ke.get_official_eval_result(gt, dt, CLASSES, PR_detail_dict=d2)
    assert a[0] == b[0]
    assert all(np.float64(a[1][k]).tobytes() == np.float64(b[1][k]).tobytes() for k in a[1])
    for k in d1:
        assert d1[k].tobytes() == d2[k].tobytes()


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_calculate_iou_partly_blocks(ke, kz, metric):
    # the reference's call order (dt first): per-part [sum dt, sum gt] matrices and each frame's block of them
    gt, dt = R.annos_from_npz(kz, "gt_"), R.annos_from_npz(kz, "dt_")
    overlaps, parted, dt_num, gt_num = ke.calculate_iou_partly(dt, gt, metric, num_parts=7)
    assert len(parted) == 8 and len(overlaps) == len(gt)                 # 100 frames: 7 parts of 14 and one of 2
    assert sum(p.shape[0] for p in parted) == dt_num.sum() and sum(p.shape[1] for p in parted) == gt_num.sum()
    want = R.frame_overlaps(gt, dt, metric)
    tol = 0.0 if metric == 0 else 5e-4       # float32 rotated overlaps at up to 70 m (test_stages_vs_numpy_large)
    for f, (got, ref) in enumerate(zip(overlaps, want)):
        assert got.shape == ref.shape, f
        assert np.abs(got - ref).max(initial=0) <= tol, f
