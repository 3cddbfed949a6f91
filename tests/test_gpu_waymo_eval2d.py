"""GPU: the BEV-protocol Waymo metrics (cpd_amd.waymo_eval2d, cpd_waymo_iou_bev in csrc/waymo_eval.hip) against closed
forms, the 3-D kernel where the two must and must not agree, the independent restatement (tests/ref_waymo_eval2d.py), a
frame worked out by hand, and the threshold-set parameter of cpd_amd.waymo_eval.evaluate_arrays on both box types."""
import math

import numpy as np
import pytest

import ref_waymo_eval as R3
import ref_waymo_eval2d as R

pytestmark = pytest.mark.gpu
COLS = [0, 1, 3, 4, 6]
CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
THRESHOLD_SETS = [(0.7, .5, .5, .5), (0.5, .3, .3, .3), (0.3, .3, .3, .3)]


@pytest.fixture(scope="module")
def we(hip):
    from cpd_amd import waymo_eval
    return waymo_eval


@pytest.fixture(scope="module")
def w2(hip):
    from cpd_amd import waymo_eval2d
    return waymo_eval2d


@pytest.fixture(scope="module")
def wz(golden):
    return golden("waymo_eval")


def _offsets(counts, dtype):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(dtype)


def gpu_iou_blocks(pd_sets, gt_sets, entry="cpd_waymo_iou_bev"):
    """One call of the entry point on problems given as lists of [n, width] box arrays: the [n_pd, n_gt] float64 blocks."""
    import torch
    from cpd_amd import _lib
    width = 5 if entry == "cpd_waymo_iou_bev" else 7
    n_pd, n_gt = [len(p) for p in pd_sets], [len(g) for g in gt_sets]
    pair_off = _offsets(np.array(n_pd) * np.array(n_gt), np.int64)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    pd = dev(np.concatenate([np.asarray(p, np.float32).reshape(-1, width) for p in pd_sets]), np.float32)
    gt = dev(np.concatenate([np.asarray(g, np.float32).reshape(-1, width) for g in gt_sets]), np.float32)
    d_po, d_go, d_pair = dev(_offsets(n_pd, np.int32), np.int32), dev(_offsets(n_gt, np.int32), np.int32), dev(pair_off, np.int64)
    out = torch.full((max(int(pair_off[-1]), 1),), -7.0, dtype=torch.float64, device="cuda")
    P = _lib.ptr
    _lib.check(getattr(_lib.lib(), entry)(P(pd), P(gt), P(d_po), P(d_go), P(d_pair), len(n_pd), int(pair_off[-1]), P(out),
                                          _lib.stream()), entry)
    host = out.cpu().numpy()
    return [host[pair_off[q]:pair_off[q + 1]].reshape(n_pd[q], n_gt[q]) for q in range(len(n_pd))]


# ---- IoU ------------------------------------------------------------------------------------------------------------

def test_iou_closed_forms(w2):
    a = [np.array(c[0], np.float32)[None] for c in R.CLOSED_FORMS]
    b = [np.array(c[1], np.float32)[None] for c in R.CLOSED_FORMS]
    want = np.array([c[2] for c in R.CLOSED_FORMS])
    for first, second in ((a, b), (b, a)):
        got = np.array([blk[0, 0] for blk in gpu_iou_blocks(first, second)])
        for g, w in zip(got, want):
            print("got %.17g want %.17g" % (g, w))
        assert np.abs(got - want).max() <= 1e-12


def test_z_disjoint_pair_overlaps_in_bev_only(w2):
    a = np.array([[3.0, 4.0, 0.5, 4.0, 2.0, 1.5, 0.7]], np.float32)
    b = a.copy()
    b[0, 2] += 10.0                                                   # the same footprint, 10 m higher
    assert gpu_iou_blocks([a], [b], "cpd_waymo_iou")[0][0, 0] == 0.0
    assert gpu_iou_blocks([a[:, COLS]], [b[:, COLS]])[0][0, 0] == 1.0


def random_boxes7(rng, n, centre=(20.0, -35.0), radius=4.0):
    """Sizes 0.3 .. 6 m both ways, every heading in +-2 pi, centres in a disc: any two lie within 8 m of each other."""
    r, phi = radius * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(-np.pi, np.pi, n)
    out = np.zeros((n, 7), np.float32)
    out[:, 0], out[:, 1] = centre[0] + r * np.cos(phi), centre[1] + r * np.sin(phi)
    out[:, 2] = rng.uniform(-1, 1, n)
    out[:, 3], out[:, 4] = rng.uniform(0.3, 6.0, n), rng.uniform(0.3, 6.0, n)
    out[:, 5] = rng.uniform(0.5, 2.5, n)
    out[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, n)
    return out


def test_same_height_pairs_agree_with_the_3d_kernel(w2):
    rng = np.random.default_rng(17)
    pd, gt = random_boxes7(rng, 70), random_boxes7(rng, 66)
    pd[:, 2], gt[:, 2], pd[:, 5], gt[:, 5] = 0.4, 0.4, 1.7, 1.7       # equal cz and dz: the height cancels
    bev = gpu_iou_blocks([pd[:, COLS]], [gt[:, COLS]])[0]
    full = gpu_iou_blocks([pd], [gt], "cpd_waymo_iou")[0]
    print("max |bev - 3d| %.3g over %d overlapping pairs" % (np.abs(bev - full).max(), np.count_nonzero(full > 0)))
    assert np.count_nonzero(full > 0) >= 70 * 66 // 3
    assert np.abs(bev - full).max() <= 1e-12


# shapes with empty problems in between: consecutive pair offsets are equal there
IOU_SHAPES = [(1, 1), (0, 5), (63, 65), (5, 0), (65, 63), (0, 0), (130, 40)]


def test_iou_blocks_vs_restatement(w2):
    rng = np.random.default_rng(5)
    pd_sets = [random_boxes7(rng, r)[:, COLS] for r, _ in IOU_SHAPES]
    gt_sets = [random_boxes7(rng, c)[:, COLS] for _, c in IOU_SHAPES]
    pd_sets[0][0] = gt_sets[0][0] + np.array([0.2, 0.1, 0, 0, 0.1], np.float32)          # the 1 x 1 block overlaps
    got = gpu_iou_blocks(pd_sets, gt_sets)          # one call: the segment offsets are exercised
    pairs, overlapping = 0, 0
    for (r, c), p, g, blk in zip(IOU_SHAPES, pd_sets, gt_sets, got):
        assert blk.shape == (r, c)
        want = R.iou_matrix_bev(p, g)
        pairs += r * c
        overlapping += int(np.count_nonzero(want > 0))
        err = np.abs(blk - want).max(initial=0)
        print("block %d x %d: max |diff| %.3g" % (r, c, err))
        assert err <= 1e-7, (r, c)                  # the tolerance of the 3-D blocks (test_gpu_waymo_eval.py)
    print("%d of %d pairs overlap" % (overlapping, pairs))
    assert 3 * overlapping >= pairs


def test_iou_degenerate_rows_give_a_finite_zero(w2):
    base = np.array([3.0, 4.0, 4.0, 2.0, 0.3], np.float32)
    rows = []
    for col in range(5):
        for v in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            b = base.copy()
            b[col] = v
            rows.append(b)
    for dx, dy in ((0.0, 2.0), (4.0, 0.0), (0.0, 0.0), (-4.0, 2.0), (4.0, -2.0), (-4.0, -2.0)):
        b = base.copy()
        b[2], b[3] = dx, dy
        rows.append(b)
    rows = np.array(rows)
    as_row = gpu_iou_blocks([rows], [base[None]])[0][:, 0]
    as_col = gpu_iou_blocks([base[None]], [rows])[0][0]
    among = gpu_iou_blocks([rows], [rows])[0]
    for got in (as_row, as_col, among):
        assert np.all(np.isfinite(got))
        assert np.all(got == 0.0)
    assert gpu_iou_blocks([base[None]], [base[None]])[0][0, 0] == 1.0        # the row they were made from is a box


# ---- one frame by hand ----------------------------------------------------------------------------------------------

HEADING_OFF = 0.2


def worked_infos():
    """Three Vehicle ground truths at levels 1, 1, 2 (by point count) and four predictions: 0.9 on the first ground truth
    exactly; 0.8 on the second moved half its length along its heading -- IoU (L - L/2) / (L + L/2) = 1/3 in BEV and,
    at equal heights, in 3-D; 0.7 over the third, turned by 0.2 rad and 10 m higher: BEV IoU 0.806, 3-D IoU 0; 0.4 far away."""
    g = np.array([[10.0, 5.0, 1.0, 4.5, 2.0, 1.6, 0.1], [-20.0, 8.0, 1.0, 4.5, 2.0, 1.6, 1.2], [30.0, -10.0, 1.0, 4.0, 2.0, 1.6, 0.0]])
    p = np.array([g[0], g[1], g[2], [40.0, -30.0, 1.0, 4.5, 2.0, 1.6, 0.0]])
    p[1, 0] += 2.25 * math.cos(1.2)
    p[1, 1] += 2.25 * math.sin(1.2)
    p[2, 2] += 10.0
    p[2, 6] += HEADING_OFF
    gt = {"name": np.array(["Vehicle"] * 3), "difficulty": np.array([0, 0, 0]), "num_points_in_gt": np.array([50, 80, 3]),
          "gt_boxes_lidar": g}
    pd = {"name": np.array(["Vehicle"] * 4), "score": np.array([0.9, 0.8, 0.7, 0.4], np.float32), "boxes_lidar": p}
    return [pd], [gt]


def test_worked_case_end_to_end(we, w2):
    # BEV protocol, vehicles at 0.5. 0.9 is a TP at both levels; 0.8 (IoU 1/3) is an FP; 0.7 takes the level-2 ground
    # truth: a TP at level 2, and at level 1 neither TP nor FP; 0.4 is an FP.
    #   subset            level 1 tp fp fn      level 2 tp fp fn
    #   all four (k<=40)          1  2  1               2  2  1
    #   0.9 0.8 0.7 (k=50)        1  1  1               2  1  1
    #   none (k=100)              0  0  2               0  0  3
    detail = {}
    got = w2.OpenPCDetWaymoDetectionMetricsEstimator().waymo_evaluation(*worked_infos(), CLASSES, fake_gt_infos=False, detail=detail)
    c = detail["counts"][0]
    np.testing.assert_array_equal(c[0][[0, 50, 100]], [[1, 2, 1], [1, 1, 1], [0, 0, 2]])
    np.testing.assert_array_equal(c[1][[0, 50, 100]], [[2, 2, 1], [2, 1, 1], [0, 0, 3]])
    # level 1: every operating point has recall 1/2, the best precision there is 1 (0.9 alone): AP = 1/2; the TP's heading
    # is exact, so APH = AP. level 2: recall 1/3 with precision 1 (0.9 alone), recall 2/3 with precision 2/3 (the three
    # best): AP = 1/3 + 1/3 * 2/3. With t = 1 - 0.2 / pi the heading accuracy of the turned TP, the heading-weighted points
    # are (1/3, 1), (1/3, 1/2), ((1 + t) / 3, (1 + t) / 3), ((1 + t) / 3, (1 + t) / 4): APH = 1/3 + t/3 * (1 + t)/3.
    t = 1.0 - float(np.float32(HEADING_OFF)) / math.pi
    want = {"LEVEL_1/AP": 0.5, "LEVEL_1/APH": 0.5, "LEVEL_2/AP": 1.0 / 3.0 + 2.0 / 9.0, "LEVEL_2/APH": 1.0 / 3.0 + t / 3.0 * (1.0 + t) / 3.0}
    for k, v in want.items():
        print("2-D %s: got %.15g want %.15g" % (k, got["OBJECT_TYPE_TYPE_VEHICLE_" + k][0], v))
        assert abs(got["OBJECT_TYPE_TYPE_VEHICLE_" + k][0] - v) <= 1e-12, k
    assert abs(detail["ha"][0, 1, 0] - (1.0 + t)) <= 1e-12
    assert all(v == [0.0] for k, v in got.items() if "VEHICLE" not in k)

    # 3-D protocol, vehicles at 0.7: the prediction 10 m above the third ground truth no longer touches it -- one more FP
    # at every cut-off that admits it, one TP fewer at level 2.
    #   all four                  1  3  1               1  3  2
    #   0.9 0.8 0.7               1  2  1               1  2  2
    #   none                      0  0  2               0  0  3
    detail3 = {}
    got3 = we.OpenPCDetWaymoDetectionMetricsEstimator().waymo_evaluation(*worked_infos(), CLASSES, fake_gt_infos=False, detail=detail3)
    c = detail3["counts"][0]
    np.testing.assert_array_equal(c[0][[0, 50, 100]], [[1, 3, 1], [1, 2, 1], [0, 0, 2]])
    np.testing.assert_array_equal(c[1][[0, 50, 100]], [[1, 3, 2], [1, 2, 2], [0, 0, 3]])
    for k, v in {"LEVEL_1/AP": 0.5, "LEVEL_1/APH": 0.5, "LEVEL_2/AP": 1.0 / 3.0, "LEVEL_2/APH": 1.0 / 3.0}.items():
        assert abs(got3["OBJECT_TYPE_TYPE_VEHICLE_" + k][0] - v) <= 1e-12, k


# ---- the scene set --------------------------------------------------------------------------------------------------

def subset_matchings(w, score):
    out, prev = [], None
    for k in range(101):
        idx = np.nonzero(score >= R.CUTOFFS[k])[0]
        if prev is not None and len(idx) == prev:
            continue
        prev = len(idx)
        out.append(frozenset((int(idx[i]), j) for i, j in R.optimal_pairs(w[idx])))
    return out


def assert_stable(blocks, scores, thresholds, rng):
    """The input condition test_gpu_waymo_eval.py puts on its problems, asserted on the CPU for these: no IoU within 1e-4
    of its threshold and every cut-off's optimal matching unchanged under five random +-1e-7 perturbations of the weights,
    so the restatement's counts do not hang on a tie that the kernel may break the other way."""
    for f, t, order, gi, iou in blocks:
        if iou.size == 0:
            continue
        thr = thresholds[t - 1]
        assert np.abs(iou - thr).min() >= 1e-4, (f, t)
        w = np.where(iou >= thr, iou, 0.0)
        score = np.asarray(scores[order], np.float32)
        base = subset_matchings(w, score)
        for _ in range(5):
            wp = np.where(w > 0, w + rng.uniform(-1e-7, 1e-7, w.shape), 0.0)
            assert subset_matchings(wp, score) == base, "frame %d type %d has a near-tie" % (f, t)


@pytest.fixture(scope="module")
def scene_run(w2, wz):
    est = w2.OpenPCDetWaymoDetectionMetricsEstimator()
    classes = [str(c) for c in wz["class_names"]]
    detail = {}
    result = est.waymo_evaluation(*R3.infos_from_flat(wz), classes, detail=detail)
    return est, classes, result, detail


def test_scene_set_vs_restatement(w2, wz, scene_run):
    _, classes, result, detail = scene_run
    want, counts, ha, blocks = R.waymo_evaluation(*R3.infos_from_flat(wz), classes)
    pd = R.generate_waymo_type_results(R3.infos_from_flat(wz)[0], classes, False)
    scores = R.mask_by_distance(100, pd[1], pd[3])[1]
    assert_stable(blocks, scores, R.IOU_THRESHOLDS, np.random.default_rng(1002))
    assert detail["counts"].dtype == np.int64 and detail["counts"].shape == (4, 2, 101, 3)
    for b in np.argwhere(detail["counts"] != counts)[:5]:
        print("counts%s: got %d want %d" % (tuple(b), detail["counts"][tuple(b)], counts[tuple(b)]))
    np.testing.assert_array_equal(detail["counts"], counts)
    assert np.all(np.abs(detail["ha"] - ha) <= 1e-9 * (1 + np.abs(ha)))
    assert list(result) == list(want) and len(want) == 16
    for k in want:
        assert isinstance(result[k], list) and len(result[k]) == 1 and type(result[k][0]) is float
        print("%s: got %.15g want %.15g" % (k, result[k][0], want[k][0]))
        assert abs(result[k][0] - want[k][0]) <= 1e-12, k
    assert result["OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/AP"][0] > 0.1 and counts[:, 1, 0, 0].sum() > 50


def test_scene_set_in_chunks_is_identical(w2, wz, scene_run):
    est, classes, result, detail = scene_run
    for kw in (dict(chunk_frames=1), dict(pair_budget=40), dict(chunk_frames=7, pair_budget=1)):
        chunked = {}
        again = est.waymo_evaluation(*R3.infos_from_flat(wz), classes, detail=chunked, **kw)
        np.testing.assert_array_equal(chunked["counts"], detail["counts"])
        assert chunked["ha"].tobytes() == detail["ha"].tobytes(), kw
        assert again == result


def test_raw_scores_above_one_go_through_the_sigmoid(w2, wz, capsys):
    est = w2.OpenPCDetWaymoDetectionMetricsEstimator()
    classes = [str(c) for c in wz["class_names"]]
    detail = {}
    got = est.waymo_evaluation(*R3.infos_from_flat(wz, "lg_"), classes, detail=detail)
    assert "Warning: Waymo evaluation only supports normalized scores" in capsys.readouterr().out
    want, counts, ha, _ = R.waymo_evaluation(*R3.infos_from_flat(wz, "lg_"), classes)
    np.testing.assert_array_equal(detail["counts"], counts)
    for k in want:
        assert abs(got[k][0] - want[k][0]) <= 1e-12, k


def test_empty_prediction_set_gives_zeros(w2):
    _, gt_infos = worked_infos()
    empty = [{"name": np.zeros(0, "<U16"), "score": np.zeros(0, np.float32), "boxes_lidar": np.zeros((0, 7))}]
    detail = {}
    got = w2.OpenPCDetWaymoDetectionMetricsEstimator().waymo_evaluation(empty, gt_infos, CLASSES, fake_gt_infos=False, detail=detail)
    assert all(v == [0.0] for v in got.values()) and len(got) == 16
    np.testing.assert_array_equal(detail["counts"][0, :, :, 2], np.array([[2] * 101, [3] * 101]))
    assert detail["counts"][..., :2].sum() == 0


# ---- threshold sets -------------------------------------------------------------------------------------------------

def mixed_infos():
    """A small synthetic split whose IoUs spread over every threshold, and the worked frame (a vehicle pair at 1/3)."""
    from cpd_amd.synthetic import waymo_infos
    pd_infos, gt_infos = waymo_infos(6, seed=3, n_gt=12, n_pd=30)
    pd_one, gt_one = worked_infos()
    return pd_infos + pd_one, gt_infos + gt_one


@pytest.mark.parametrize("box_type", ["TYPE_3D", "TYPE_2D"])
def test_threshold_sets_equal_separate_calls(we, w2, box_type):
    module = we if box_type == "TYPE_3D" else w2
    est = module.OpenPCDetWaymoDetectionMetricsEstimator()
    pd_infos, gt_infos = mixed_infos()
    pf, pb, pt, ps, _, _ = est.generate_waymo_type_results(pd_infos, CLASSES, is_gt=False)
    gf, gb, gt, _, _, gd = est.generate_waymo_type_results(gt_infos, CLASSES, is_gt=True, fake_gt_infos=False)
    arrays = (pf, pb, pt, ps, gf, gb, gt, gd, len(gt_infos))
    counts, ha = we.evaluate_arrays(*arrays, box_type=box_type, iou_thresholds=THRESHOLD_SETS)
    assert counts.shape == (3, 4, 2, 101, 3) and counts.dtype == np.int64 and ha.shape == (3, 4, 2, 101) and ha.dtype == np.float64
    for s, one in enumerate(THRESHOLD_SETS):
        c, h = we.evaluate_arrays(*arrays, box_type=box_type, iou_thresholds=one)
        assert c.shape == (4, 2, 101, 3) and h.shape == (4, 2, 101)
        np.testing.assert_array_equal(counts[s], c)
        assert ha[s].tobytes() == h.tobytes(), s
    for i, j in ((0, 1), (1, 2), (0, 2)):                             # the sets are told apart by this input
        assert not np.array_equal(counts[i], counts[j]), (i, j)
    own = 0 if box_type == "TYPE_3D" else 1                           # the default is the protocol's own set
    c, h = we.evaluate_arrays(*arrays, box_type=box_type)
    np.testing.assert_array_equal(c, counts[own])
    assert h.tobytes() == ha[own].tobytes()
    # chunks continue every set's totals
    c, h = we.evaluate_arrays(*arrays, box_type=box_type, iou_thresholds=THRESHOLD_SETS, chunk_frames=2, pair_budget=50)
    np.testing.assert_array_equal(c, counts)
    assert h.tobytes() == ha.tobytes()
    # the estimator's method: one result dict per set, and waymo_evaluation itself is the protocol's own
    detail = {}
    results = est.waymo_evaluation_at(pd_infos, gt_infos, CLASSES, THRESHOLD_SETS, fake_gt_infos=False, detail=detail)
    np.testing.assert_array_equal(detail["counts"], counts)
    assert detail["ha"].tobytes() == ha.tobytes()
    assert isinstance(results, list) and len(results) == 3
    for s in range(3):
        assert results[s] == we.result_dict(counts[s], ha[s])
    assert est.waymo_evaluation(pd_infos, gt_infos, CLASSES, fake_gt_infos=False) == results[own]
    assert results[0] != results[2]
