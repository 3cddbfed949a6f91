"""tests/ref_anchor_batch.py, the host statement that cpd_anchor_assign_batch is tested against, itself against the reference's own
assign_targets output (tests/golden/anchor_head.npz), and the properties of the small case that make it a test: forced matches
below the threshold, a tie for a row's maximum, a row nothing overlaps, the class-0 wrap, an all-zero row between boxes, an
ignore label. CPU."""
import numpy as np
import pytest

import ref_anchor_batch as rab

GOLDEN_THR = {"Vehicle": (0.55, 0.4), "Pedestrian": (0.5, 0.35), "Cyclist": (0.5, 0.35)}   # make_golden.py's anchor_head section


def test_helper_reproduces_reference_assign_targets(oracle, golden):
    g = golden("anchor_head")
    sets = [np.asarray(a) for a in g["anchors_per_class"]]          # (1, H, W, 1, 2, 7) each
    got = rab.ref_anchor_batch(oracle, sets, g["gt"], rab.CLASSES, rab.CLASSES, GOLDEN_THR)
    np.testing.assert_array_equal(got["labels"], g["labels"])
    np.testing.assert_array_equal(got["gt_ious"], g["gt_ious"])
    np.testing.assert_array_equal(got["reg_weights"], g["reg_weights"])
    np.testing.assert_allclose(got["reg_targets"], g["reg_targets"], rtol=0, atol=1e-6)
    assert got["gt_max_iou"].shape == g["gt"].shape[:2] and got["n_examples"].shape == (g["gt"].shape[0], 3)
    np.testing.assert_array_equal(got["n_examples"].sum(1), (g["labels"] >= 0).sum(1))


@pytest.fixture(scope="module")
def small(oracle):
    from cpd_amd import anchor_head as ah
    cfgs = rab.small_cfgs()
    anchors, per_loc = ah.AnchorGenerator(rab.SMALL_RANGE, cfgs).generate_anchors([rab.SMALL_GRID] * 3, device="cpu")
    assert per_loc == [2, 2, 2] and all(tuple(a.shape) == (1, 9, 11, 1, 2, 7) for a in anchors)
    sets = [a.numpy() for a in anchors]
    np.testing.assert_array_equal(sets[0][0, 0, :, 0, 0, 0], np.arange(0, 21, 2, dtype=np.float32))
    np.testing.assert_array_equal(sets[0][0, :, 0, 0, 0, 1], np.arange(-10, 10.1, 2.5, dtype=np.float32))
    gt = rab.small_gt()
    assert gt.shape == (5, 8, 8)
    return sets, gt, rab.ref_anchor_batch(oracle, sets, gt, rab.CLASSES, rab.CLASSES, rab.thresholds(cfgs))


def _of_set(small, key, b, s):
    sets, _, ref = small
    return ref[key][b][rab.set_columns(sets, s)]


def test_small_case_layout_and_shapes(small):
    sets, gt, ref = small
    assert ref["labels"].shape == (5, 594) and ref["reg_targets"].shape == (5, 594, 7)
    cols = np.concatenate([rab.set_columns(sets, s) for s in range(3)])
    np.testing.assert_array_equal(np.sort(cols), np.arange(594))     # every column belongs to exactly one anchor
    # feature_map_size = anchors.shape[:2] = (1, 9): outer 9, inner 22 per set, 66 columns per outer position
    np.testing.assert_array_equal(rab.set_columns(sets, 1)[[0, 1, 21, 22, 197]], [22, 23, 43, 88, 571])
    np.testing.assert_array_equal(ref["n_examples"].sum(1), (ref["labels"] >= 0).sum(1))


def test_small_case_frame0_vehicle_forced_matches_and_a_four_way_tie(oracle, small):
    sets, gt, ref = small
    assert [r.tolist() for r in ref["rows"][0]] == [[1, 3, 5], [0, 4], [2, 6]]
    lab, iou = _of_set(small, "labels", 0, 0), _of_set(small, "gt_ious", 0, 0)
    assert int((lab > 0).sum()) == 6 and set(lab[lab > 0].tolist()) == {1}
    assert int(((lab > 0) & (iou < np.float32(0.55))).sum()) == 5    # force-matched below the matched threshold
    to_second = oracle.nearest_bev_iou(sets[0].reshape(-1, 7), gt[0, 3:4, :7])[:, 0]
    assert ref["gt_max_iou"][0, 3] > 0 and int((to_second == ref["gt_max_iou"][0, 3]).sum()) == 4
    assert (lab[to_second == ref["gt_max_iou"][0, 3]] == 1).all()


def test_small_case_frame0_second_pedestrian_overlaps_no_anchor(small):
    _, _, ref = small
    assert ref["gt_max_iou"][0, 4] == 0 and ref["gt_max_iou"][0, 0] > 0
    assert (ref["gt_max_iou"][0, 7:] == 0).all()                     # padding


def test_small_case_empty_frame_hands_one_zero_box_to_the_last_class(small):
    _, _, ref = small
    assert [r.tolist() for r in ref["rows"][2]] == [[], [], [0]]
    assert (ref["labels"][2] == 0).all() and (ref["reg_weights"][2] == 0).all() and (ref["reg_targets"][2] == 0).all()
    assert (ref["gt_ious"][2] == 0).all() and (ref["gt_max_iou"][2] == 0).all()
    assert ref["n_examples"][2].tolist() == [198, 198, 198]


def test_small_case_zero_row_between_boxes_joins_the_last_class(small):
    _, _, ref = small
    assert [r.tolist() for r in ref["rows"][3]] == [[0], [], [1, 2]]
    lab = _of_set(small, "labels", 3, 2)
    assert int((lab > 0).sum()) == 1 and int(lab.max()) == 3
    assert ref["gt_max_iou"][3, 1] == 0 and ref["gt_max_iou"][3, 2] > 0


def test_small_case_frame4_box_off_the_grid_and_a_forced_pedestrian_with_an_ignore_label(small):
    _, _, ref = small
    assert [r.tolist() for r in ref["rows"][4]] == [[0], [1], []]
    assert (_of_set(small, "labels", 4, 0) == 0).all() and ref["gt_max_iou"][4, 0] == 0
    lab, iou = _of_set(small, "labels", 4, 1), _of_set(small, "gt_ious", 4, 1)
    assert int((lab > 0).sum()) == 1 and int((lab == -1).sum()) == 1
    assert abs(float(iou[lab > 0][0]) - 0.524) < 5e-4 and iou[lab > 0][0] == ref["gt_max_iou"][4, 1]
    assert ref["n_examples"][4].tolist() == [198, 197, 198]


def test_small_case_norm_by_num_examples_divides_by_the_pair_count(oracle, small):
    sets, gt, ref = small
    normed = rab.ref_anchor_batch(oracle, sets, gt, rab.CLASSES, rab.CLASSES, rab.thresholds(rab.small_cfgs()), True)
    np.testing.assert_array_equal(normed["labels"], ref["labels"])
    w = normed["reg_weights"][4][rab.set_columns(sets, 1)]
    assert w[w > 0].tolist() == [np.float32(1.0) / np.float32(197)]
