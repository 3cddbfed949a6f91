"""Host half of cpd_amd.waymo_eval (no GPU): preprocessing, distance mask and the AP integration against the independent
restatement (tests/ref_waymo_eval.py) and the golden (tests/golden/waymo_eval.npz); result layout; errors."""
import copy

import numpy as np
import pytest

import ref_waymo_eval as R


@pytest.fixture(scope="module")
def we():
    from cpd_amd import waymo_eval
    return waymo_eval


@pytest.fixture(scope="module")
def wz(golden):
    return golden("waymo_eval")


@pytest.fixture(scope="module")
def class_names(wz):
    return [str(c) for c in wz["class_names"]]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("prefix", ["", "lg_"])
def test_generate_results_match_restatement(we, wz, class_names, prefix):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    pd_infos, gt_infos = R.infos_from_flat(wz, prefix)
    _same(est.generate_waymo_type_results(pd_infos, class_names, is_gt=False),
          R.generate_waymo_type_results(pd_infos, class_names, False))
    for fake in (True, False):
        got = est.generate_waymo_type_results(gt_infos, class_names, is_gt=True, fake_gt_infos=fake)
        _same(got, R.generate_waymo_type_results(gt_infos, class_names, True, fake))
        frame_id, boxes, obj_type, score, nlz, difficulty = got
        assert frame_id.dtype == np.int64 and difficulty.dtype == np.int8 and score.dtype == np.float64
        assert set(np.unique(difficulty)) <= {1, 2}                       # 0 is decided by the point count
        assert np.all((boxes[:, 6] >= -np.pi) & (boxes[:, 6] < np.pi))    # limit_period(heading, 0.5, 2 pi)
    # boxes without points are dropped, and only the asked classes are kept
    kept = sum(int(np.count_nonzero((g["num_points_in_gt"] > 0) & np.isin(g["name"], class_names))) for g in gt_infos)
    assert len(got[0]) == kept < sum(len(g["name"]) for g in gt_infos)


def test_difficulty_rule(we):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    info = {"name": np.array(["Vehicle"] * 6), "difficulty": np.array([0, 0, 0, 0, 2, 1]),
            "num_points_in_gt": np.array([0, 1, 5, 6, 100, 3]), "gt_boxes_lidar": np.arange(42, dtype=np.float64).reshape(6, 7)}
    out = est.generate_waymo_type_results([info], ["Vehicle"], is_gt=True, fake_gt_infos=False)
    np.testing.assert_array_equal(out[5], [2, 2, 1, 2, 1])                # the box without points is gone
    np.testing.assert_array_equal(out[2], [1] * 5)
    np.testing.assert_array_equal(out[1][:, :6], info["gt_boxes_lidar"][1:, :6])


def test_fake_lidar_conversion(we):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    info = {"name": np.array(["Cyclist"]), "difficulty": np.array([0]), "num_points_in_gt": np.array([9]),
            "gt_boxes_lidar": np.array([[1.0, 2.0, 3.0, 0.5, 1.5, 2.0, 0.25]])}
    boxes = est.generate_waymo_type_results([info], ["Cyclist"], is_gt=True, fake_gt_infos=True)[1]
    want = [1.0, 2.0, 4.0, 1.5, 0.5, 2.0, -(0.25 + np.pi / 2)]
    np.testing.assert_allclose(boxes[0], want, rtol=0, atol=1e-15)
    assert est.generate_waymo_type_results([info], ["Cyclist"], is_gt=True)[2][0] == 4      # the list index is the type id


def test_inputs_are_not_modified(we, wz, class_names):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    pd_infos, gt_infos = R.infos_from_flat(wz)
    before = copy.deepcopy((pd_infos, gt_infos))
    est.generate_waymo_type_results(pd_infos, class_names, is_gt=False)
    est.generate_waymo_type_results(gt_infos, class_names, is_gt=True, fake_gt_infos=True)
    for now, then in zip(pd_infos + gt_infos, before[0] + before[1]):
        assert list(now) == list(then)
        for k in now:
            assert now[k].dtype == then[k].dtype
            np.testing.assert_array_equal(now[k], then[k])


def test_missing_point_counts_raise(we):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    info = {"name": np.array(["Vehicle"]), "difficulty": np.array([0]), "gt_boxes_lidar": np.zeros((1, 7))}
    with pytest.raises(NotImplementedError):
        est.generate_waymo_type_results([info], ["Vehicle"], is_gt=True)


def test_mask_by_distance(we):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    rng = np.random.default_rng(3)
    boxes = rng.uniform(-120, 120, (200, 7))
    boxes[0, :2], boxes[1, :2] = (100.4, 0.0), (0.0, 100.5)               # inside / on the bound (strict <)
    extra, flags = np.arange(200), rng.uniform(size=200) < 0.5
    got = est.mask_by_distance(100, boxes, extra, flags)
    want = R.mask_by_distance(100, boxes, extra, flags)
    assert isinstance(got, tuple) and len(got) == 3
    _same(got, want)
    assert 0 in got[1] and 1 not in got[1]


CURVES = {
    # tp, fp, fn per cut-off
    "monotone": ([10, 9, 8, 6, 3, 0], [10, 6, 3, 1, 0, 0], [0, 1, 2, 4, 7, 10]),
    "non_monotone": ([10, 9, 8, 6, 3, 0], [2, 6, 1, 3, 0, 0], [0, 1, 2, 4, 7, 10]),
    "duplicate_recall": ([6, 6, 6, 3, 3, 0], [9, 4, 6, 2, 0, 0], [0, 0, 0, 3, 3, 6]),
    "all_zero": ([0] * 6, [0] * 6, [0] * 6),
    "no_ground_truth": ([0] * 4, [5, 3, 1, 0], [0] * 4),
    "no_detection": ([0] * 4, [0] * 4, [7] * 4),
}


@pytest.mark.parametrize("name", sorted(CURVES))
def test_average_precision_vs_restatement(we, name):
    tp, fp, fn = CURVES[name]
    got = we.average_precision(tp, fp, fn)
    assert isinstance(got, float) and 0.0 <= got <= 1.0
    assert abs(got - R.average_precision(tp, fp, fn)) <= 1e-12
    ha = [0.8 * t for t in tp]
    assert abs(we.average_precision(tp, fp, fn, ha) - R.average_precision(tp, fp, fn, ha)) <= 1e-12
    if name in ("all_zero", "no_ground_truth", "no_detection"):
        assert got == 0.0


def test_average_precision_by_hand(we):
    # monotone: recalls 0.3, 0.6, 0.8, 0.9, 1.0 with precisions 1, 6/7, 8/11, 0.6, 0.5
    tp, fp, fn = CURVES["monotone"]
    want = 0.3 * 1 + 0.3 * 6 / 7 + 0.2 * 8 / 11 + 0.1 * 0.6 + 0.1 * 0.5
    assert abs(we.average_precision(tp, fp, fn) - want) <= 1e-12
    # non-monotone: the precision at a recall is the best one at that recall or beyond
    tp, fp, fn = CURVES["non_monotone"]
    want = 0.3 * 1 + 0.3 * 8 / 9 + 0.2 * 8 / 9 + 0.1 * 10 / 12 + 0.1 * 10 / 12
    assert abs(we.average_precision(tp, fp, fn) - want) <= 1e-12


def worked_counts():
    """One frame, two level-1 Vehicle ground truths; predictions scored 0.9 (matches one), 0.8 (nothing), 0.7 (the other)."""
    score = np.array([0.9, 0.8, 0.7], np.float32)
    matches = np.array([True, False, True])
    tp = np.array([np.count_nonzero(matches & (score >= c)) for c in R.CUTOFFS])
    fp = np.array([np.count_nonzero(~matches & (score >= c)) for c in R.CUTOFFS])
    return tp, fp, 2 - tp


def test_worked_case(we):
    tp, fp, fn = worked_counts()
    points = {(t / 2, t / (t + f) if t + f else 0.0) for t, f in zip(tp, fp)}
    assert points == {(1.0, 2 / 3), (0.5, 0.5), (0.5, 1.0), (0.0, 0.0)}
    assert abs(we.average_precision(tp, fp, fn) - (0.5 * 1 + 0.5 * 2 / 3)) <= 1e-15


def test_result_dict_layout_and_golden_values(we, wz):
    got = we.result_dict(wz["counts"], wz["ha"])
    assert list(got) == [str(k) for k in wz["keys"]]
    assert list(got) == ['OBJECT_TYPE_TYPE_%s_LEVEL_%d/%s' % (t, l, m) for t in ('VEHICLE', 'PEDESTRIAN', 'SIGN', 'CYCLIST')
                         for l in (1, 2) for m in ('AP', 'APH')]
    for (k, v), want in zip(got.items(), wz["values"]):
        assert isinstance(v, list) and len(v) == 1 and type(v[0]) is float, k       # the caller reads ap_dict[key][0]
        assert 0.0 <= v[0] <= 1.0
        assert abs(v[0] - want) <= 1e-12, k
    # the golden set has operating points: not everything is zero, and the type without ground truths is
    assert got['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/AP'][0] > 0.1
    assert got['OBJECT_TYPE_TYPE_SIGN_LEVEL_2/AP'][0] == 0.0


def test_build_config_and_constants(we):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    assert est.WAYMO_CLASSES == ['unknown', 'Vehicle', 'Pedestrian', 'Truck', 'Cyclist']
    cfg = est.build_config()
    assert isinstance(cfg, dict)
    assert cfg['iou_thresholds'] == [0.0, 0.7, 0.5, 0.5, 0.5]
    assert cfg['matcher_type'] == 'TYPE_HUNGARIAN' and cfg['difficulties'] == {'levels': [1, 2]}
    assert cfg['score_cutoffs'] == [x * 0.01 for x in range(100)] + [1.0]
    np.testing.assert_array_equal(we.SCORE_CUTOFFS, np.array(cfg['score_cutoffs']).astype(np.float32))
    np.testing.assert_array_equal(we.SCORE_CUTOFFS, R.CUTOFFS)


def test_errors(we, wz, class_names, monkeypatch):
    import torch
    from cpd_amd._lib import CpdHipError
    with pytest.raises(ValueError):
        we.average_precision([1, 2], [1], [0, 0])
    with pytest.raises(ValueError):
        we.average_precision([1, 2], [1, 1], [0, 0], ha=[0.5])
    ok = dict(pd_frame=np.zeros(2, np.int64), pd_boxes=np.ones((2, 7)), pd_type=np.ones(2), pd_score=np.full(2, 0.5),
              gt_frame=np.zeros(1, np.int64), gt_boxes=np.ones((1, 7)), gt_type=np.ones(1), gt_difficulty=np.ones(1), n_frames=1)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for bad, exc in ((dict(pd_boxes=np.ones((2, 6))), ValueError), (dict(gt_boxes=np.ones(7)), ValueError),
                     (dict(pd_score=np.full(3, 0.5)), ValueError), (dict(gt_difficulty=np.ones((1, 1))), ValueError),
                     (dict(pd_frame=np.array([0, 1])), ValueError), (dict(pd_score=np.array([0.5, np.nan])), ValueError),
                     (dict(pd_boxes=np.full((2, 7), "x")), TypeError), (dict(gt_type=np.array(["Vehicle"])), TypeError)):
        with pytest.raises(exc):
            we.evaluate_arrays(**dict(ok, **bad))
    # well-formed input and no GPU: an error, never a CPU fallback
    with pytest.raises(CpdHipError):
        we.evaluate_arrays(**ok)
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    pd_infos, gt_infos = R.infos_from_flat(wz, "lg_")
    with pytest.raises(CpdHipError):
        est.waymo_evaluation(pd_infos, gt_infos, class_names)
    with pytest.raises(AssertionError):
        est.waymo_evaluation(pd_infos[:-1], gt_infos, class_names)
