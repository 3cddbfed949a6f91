"""Host half of cpd_amd.waymo_eval2d (no GPU): the 2-D preprocessing and the distance mask against the reference's own
lines (tests/golden/waymo_eval2d.npz, made by make_waymo_eval2d_golden.py), the metric config, the argument errors of the
box_type / iou_thresholds parameters, and the restatement's rectangle IoU (tests/ref_waymo_eval2d.py) on closed forms."""
import copy

import numpy as np
import pytest

import ref_waymo_eval as R3
import ref_waymo_eval2d as R

CLOSED_FORMS = R.CLOSED_FORMS


@pytest.fixture(scope="module")
def w2():
    from cpd_amd import waymo_eval2d
    return waymo_eval2d


@pytest.fixture(scope="module")
def wz(golden):
    return golden("waymo_eval")


@pytest.fixture(scope="module")
def g2(golden):
    return golden("waymo_eval2d")


@pytest.fixture(scope="module")
def class_names(wz):
    return [str(c) for c in wz["class_names"]]


def _same(got, fixture, stem, n):
    assert len(got) == n
    for i, x in enumerate(got):
        want = fixture["%s_%d" % (stem, i)]
        assert x.dtype == want.dtype and x.shape == want.shape, (stem, i, x.dtype, want.dtype, x.shape, want.shape)
        np.testing.assert_array_equal(x, want)


@pytest.mark.parametrize("prefix", ["", "lg_"])
def test_generate_results_and_mask_equal_the_reference(w2, wz, g2, class_names, prefix):
    est = w2.OpenPCDetWaymoDetectionMetricsEstimator()
    pd_infos, gt_infos = R3.infos_from_flat(wz, prefix)
    before = copy.deepcopy((pd_infos, gt_infos))
    pd = est.generate_waymo_type_results(pd_infos, class_names, is_gt=False)
    fake = est.generate_waymo_type_results(gt_infos, class_names, is_gt=True, fake_gt_infos=True)
    plain = est.generate_waymo_type_results(gt_infos, class_names, is_gt=True, fake_gt_infos=False)
    _same(pd, g2, prefix + "pd", 6)
    _same(fake, g2, prefix + "gt_fake", 6)
    _same(plain, g2, prefix + "gt_plain", 6)
    assert pd[1].shape[1] == 5 and fake[1].shape[1] == 5
    assert np.all((fake[1][:, 4] >= -np.pi) & (fake[1][:, 4] < np.pi))        # limit_period(heading, 0.5, 2 pi)
    assert not np.array_equal(fake[1], plain[1])                              # the conversion ran before the slice
    _same(est.mask_by_distance(50, pd[1], pd[0], pd[2], pd[3], pd[4]), g2, prefix + "pd_near", 5)
    _same(est.mask_by_distance(50, fake[1], fake[0], fake[2], fake[3], fake[5]), g2, prefix + "gt_near", 5)
    # the restatement the GPU tests compare with says the same
    _same(R.generate_waymo_type_results(pd_infos, class_names, False), g2, prefix + "pd", 6)
    _same(R.generate_waymo_type_results(gt_infos, class_names, True, True), g2, prefix + "gt_fake", 6)
    _same(R.generate_waymo_type_results(gt_infos, class_names, True, False), g2, prefix + "gt_plain", 6)
    # and the caller's infos are as they were
    for now, then in zip(pd_infos + gt_infos, before[0] + before[1]):
        assert list(now) == list(then)
        for k in now:
            assert now[k].dtype == then[k].dtype
            np.testing.assert_array_equal(now[k], then[k])


def test_slice_follows_the_fake_lidar_conversion(w2):
    est = w2.OpenPCDetWaymoDetectionMetricsEstimator()
    info = {"name": np.array(["Cyclist"]), "difficulty": np.array([0]), "num_points_in_gt": np.array([9]),
            "gt_boxes_lidar": np.array([[1.0, 2.0, 3.0, 0.5, 1.5, 2.0, 0.25]])}
    out = est.generate_waymo_type_results([info], ["Cyclist"], is_gt=True, fake_gt_infos=True)
    np.testing.assert_allclose(out[1], [[1.0, 2.0, 1.5, 0.5, -(0.25 + np.pi / 2)]], rtol=0, atol=1e-15)   # (x, y, l, w, heading)
    assert out[2][0] == 4
    out = est.generate_waymo_type_results([info], ["Cyclist"], is_gt=True, fake_gt_infos=False)
    np.testing.assert_array_equal(out[1], [[1.0, 2.0, 0.5, 1.5, 0.25]])


def test_difficulty_rule_and_missing_point_counts(w2):
    est = w2.OpenPCDetWaymoDetectionMetricsEstimator()
    info = {"name": np.array(["Vehicle"] * 6), "difficulty": np.array([0, 0, 0, 0, 2, 1]),
            "num_points_in_gt": np.array([0, 1, 5, 6, 100, 3]), "gt_boxes_lidar": np.arange(42, dtype=np.float64).reshape(6, 7)}
    out = est.generate_waymo_type_results([info], ["Vehicle"], is_gt=True, fake_gt_infos=False)
    np.testing.assert_array_equal(out[5], [2, 2, 1, 2, 1])                # the box without points is gone
    np.testing.assert_array_equal(out[1][:, :4], info["gt_boxes_lidar"][1:][:, [0, 1, 3, 4]])
    del info["num_points_in_gt"]
    with pytest.raises(NotImplementedError):
        est.generate_waymo_type_results([info], ["Vehicle"], is_gt=True)


def test_build_config_and_surface(w2):
    from cpd_amd import waymo_eval
    est = w2.OpenPCDetWaymoDetectionMetricsEstimator()
    assert w2.OpenPCDetWaymoDetectionMetricsEstimator.WAYMO_CLASSES == ['unknown', 'Vehicle', 'Pedestrian', 'Truck', 'Cyclist']
    cfg = est.build_config()
    assert isinstance(cfg, dict)
    assert cfg['iou_thresholds'] == [0.0, 0.5, 0.3, 0.3, 0.3]
    assert cfg['box_type'] == 'TYPE_2D'
    assert cfg['score_cutoffs'] == [x * 0.01 for x in range(100)] + [1.0] and len(cfg['score_cutoffs']) == 101
    assert cfg['matcher_type'] == 'TYPE_HUNGARIAN' and cfg['difficulties'] == {'levels': [1, 2]}
    assert cfg['breakdown_generator_ids'] == ['OBJECT_TYPE']
    assert w2.IOU_THRESHOLDS == (0.5, 0.3, 0.3, 0.3) == R.IOU_THRESHOLDS
    for name in ("generate_waymo_type_results", "build_config", "mask_by_distance", "waymo_evaluation", "waymo_evaluation_at"):
        assert callable(getattr(est, name)), name
    assert callable(w2.main) and w2.limit_period(3 * np.pi / 2, 0.5, 2 * np.pi) == pytest.approx(-np.pi / 2)
    assert w2.result_dict is waymo_eval.result_dict and w2.average_precision is waymo_eval.average_precision
    # the 3-D estimator's config is what it was
    cfg3 = waymo_eval.OpenPCDetWaymoDetectionMetricsEstimator().build_config()
    assert cfg3['iou_thresholds'] == [0.0, 0.7, 0.5, 0.5, 0.5] and cfg3['box_type'] == 'TYPE_3D'


def test_argument_errors(w2, wz, class_names, monkeypatch):
    import torch
    from cpd_amd import waymo_eval
    from cpd_amd._lib import CpdHipError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # whatever is not rejected ends at the device

    def args(width, **kw):
        base = dict(pd_frame=np.zeros(2, np.int64), pd_boxes=np.ones((2, width)), pd_type=np.ones(2), pd_score=np.full(2, 0.5),
                    gt_frame=np.zeros(1, np.int64), gt_boxes=np.ones((1, width)), gt_type=np.ones(1), gt_difficulty=np.ones(1),
                    n_frames=1)
        return dict(base, **kw)
    # row width follows the box type
    for bad in (args(7, box_type='TYPE_2D'), args(5), args(5, box_type='TYPE_3D'), args(5, box_type='TYPE_2D', gt_boxes=np.ones((1, 7))),
                args(5, box_type='TYPE_2D', pd_boxes=np.ones(5))):
        with pytest.raises(ValueError, match="boxes must be"):
            waymo_eval.evaluate_arrays(**bad)
    for box_type in ('TYPE_BEV', 'type_2d', '2D', None, 2):
        with pytest.raises(ValueError, match="box_type"):
            waymo_eval.evaluate_arrays(**args(5, box_type=box_type))
    for sets in ((0.5, 0.3, 0.3), (0.5, 0.3, 0.3, 0.3, 0.3), (0.0, 0.3, 0.3, 0.3), (0.5, 0.3, 1.5, 0.3), (0.5, -0.3, 0.3, 0.3),
                 (0.5, float("nan"), 0.3, 0.3), (), [(0.7, 0.5, 0.5, 0.5), (0.5, 0.3, 0.3)], [(0.7, 0.5, 0.5, 0.5), (0.5, 0.3, 0.3, 0.0)],
                 [()]):
        for width, box_type in ((7, 'TYPE_3D'), (5, 'TYPE_2D')):
            with pytest.raises(ValueError, match="threshold"):
                waymo_eval.evaluate_arrays(**args(width, box_type=box_type, iou_thresholds=sets))
    # well-formed: one set, several sets, a threshold of exactly 1 -- no GPU is an error, never a CPU fallback
    for kw in (dict(box_type='TYPE_2D'), dict(box_type='TYPE_2D', iou_thresholds=(1.0, 0.3, 0.3, 0.3)),
               dict(box_type='TYPE_2D', iou_thresholds=[(0.7, 0.5, 0.5, 0.5), (0.5, 0.3, 0.3, 0.3)]),
               dict(box_type='TYPE_2D', iou_thresholds=np.array([[0.7, 0.5, 0.5, 0.5]]))):
        with pytest.raises(CpdHipError):
            waymo_eval.evaluate_arrays(**args(5, **kw))
    est = w2.OpenPCDetWaymoDetectionMetricsEstimator()
    pd_infos, gt_infos = R3.infos_from_flat(wz, "lg_")
    with pytest.raises(CpdHipError):
        est.waymo_evaluation(pd_infos, gt_infos, class_names)
    with pytest.raises(ValueError, match="threshold"):                     # one set where a sequence of sets is asked for
        est.waymo_evaluation_at(pd_infos, gt_infos, class_names, (0.5, 0.3, 0.3, 0.3))
    with pytest.raises(ValueError, match="threshold"):
        est.waymo_evaluation_at(pd_infos, gt_infos, class_names, None)
    with pytest.raises(AssertionError):
        est.waymo_evaluation_at(pd_infos[:-1], gt_infos, class_names, [(0.5, 0.3, 0.3, 0.3)])


@pytest.mark.parametrize("case", range(len(CLOSED_FORMS)))
def test_restatement_iou_closed_forms(case):
    a, b, want = CLOSED_FORMS[case]
    assert abs(R.iou_pair_bev(a, b) - want) <= 1e-12
    assert abs(R.iou_pair_bev(b, a) - want) <= 1e-12
    assert abs(R.iou_matrix_bev([a], [b])[0, 0] - want) <= 1e-12


def test_restatement_iou_has_no_z_term_and_agrees_with_the_3d_one_at_equal_heights():
    rng = np.random.default_rng(11)
    for _ in range(50):
        a = np.array([*rng.uniform(-3, 3, 2), 0.4, *rng.uniform(0.5, 5, 2), 1.7, rng.uniform(-7, 7)], np.float32)
        b = np.array([*rng.uniform(-3, 3, 2), 0.4, *rng.uniform(0.5, 5, 2), 1.7, rng.uniform(-7, 7)], np.float32)
        cols = [0, 1, 3, 4, 6]
        assert abs(R.iou_pair_bev(a[cols], b[cols]) - R3.iou_pair(a, b)) <= 1e-12
        b[2] += 10.0                                                      # z-disjoint: nothing in 3-D, unchanged in BEV
        assert R3.iou_pair(a, b) == 0.0
        b[2] -= 10.0
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for col in range(5):
            x = np.array([0.0, 0.0, 2.0, 1.0, 0.3], np.float32)
            x[col] = bad
            assert R.iou_pair_bev(x, [0.0, 0.0, 2.0, 1.0, 0.3]) == 0.0 == R.iou_pair_bev([0.0, 0.0, 2.0, 1.0, 0.3], x)
