"""GPU: cpd_amd.waymo_eval (csrc/waymo_eval.hip) against closed forms, the reference's box3d_iou (golden), and the
independent restatement (tests/ref_waymo_eval.py): the IoU kernel, the matching kernel alone on synthetic IoU blocks fed
through the C-ABI, and the whole evaluation on the golden scene set."""
import ctypes

import numpy as np
import pytest

import ref_waymo_eval as R

pytestmark = pytest.mark.gpu
THRESHOLDS = (0.7, 0.5, 0.5, 0.5)


@pytest.fixture(scope="module")
def we(hip):
    from cpd_amd import waymo_eval
    return waymo_eval


@pytest.fixture(scope="module")
def wz(golden):
    return golden("waymo_eval")


def _offsets(counts, dtype):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(dtype)


def gpu_iou_blocks(pd_sets, gt_sets):
    """cpd_waymo_iou on problems given as lists of [n, 7] box arrays: the list of [n_pd, n_gt] float64 blocks."""
    import torch
    from cpd_amd import _lib
    n_pd, n_gt = [len(p) for p in pd_sets], [len(g) for g in gt_sets]
    pair_off = _offsets(np.array(n_pd) * np.array(n_gt), np.int64)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    pd = dev(np.concatenate([np.asarray(p, np.float32).reshape(-1, 7) for p in pd_sets]), np.float32)
    gt = dev(np.concatenate([np.asarray(g, np.float32).reshape(-1, 7) for g in gt_sets]), np.float32)
    d_po, d_go, d_pair = dev(_offsets(n_pd, np.int32), np.int32), dev(_offsets(n_gt, np.int32), np.int32), dev(pair_off, np.int64)
    out = torch.full((max(int(pair_off[-1]), 1),), -7.0, dtype=torch.float64, device="cuda")
    P = _lib.ptr
    _lib.check(_lib.lib().cpd_waymo_iou(P(pd), P(gt), P(d_po), P(d_go), P(d_pair), len(n_pd), int(pair_off[-1]), P(out),
                                        _lib.stream()), "cpd_waymo_iou")
    host = out.cpu().numpy()
    return [host[pair_off[q]:pair_off[q + 1]].reshape(n_pd[q], n_gt[q]) for q in range(len(n_pd))]


def gpu_match(problems):
    """cpd_waymo_match on problems (iou [R, C], score [R], difficulty [C], pd_heading [R], gt_heading [C]); problem q has
    type q % 4 + 1, the list is padded with empty problems to whole frames. Returns counts [4][2][101][3], ha [4][2][101]."""
    import torch
    from cpd_amd import _lib
    problems = list(problems)
    while len(problems) % 4:
        problems.append((np.zeros((0, 0)), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0)))
    n_pd, n_gt = [len(p[1]) for p in problems], [len(p[2]) for p in problems]
    pair_off = _offsets(np.array(n_pd) * np.array(n_gt), np.int64)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    cat = lambda i, dt: dev(np.concatenate([np.asarray(p[i], np.float64).reshape(-1) for p in problems]), dt)
    iou, score, diff, ph, gh = cat(0, np.float64), cat(1, np.float32), cat(2, np.uint8), cat(3, np.float32), cat(4, np.float32)
    if iou.numel() == 0:
        iou = torch.zeros(1, dtype=torch.float64, device="cuda")
    d_po, d_go, d_pair = dev(_offsets(n_pd, np.int32), np.int32), dev(_offsets(n_gt, np.int32), np.int32), dev(pair_off, np.int64)
    counts = torch.full((4, 2, 101, 3), -5, dtype=torch.int64, device="cuda")
    ha = torch.full((4, 2, 101), -5.0, dtype=torch.float64, device="cuda")
    lib, P = _lib.lib(), _lib.ptr
    ws_bytes = lib.cpd_waymo_match_workspace_bytes(len(problems), sum(n_pd))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    thr = (ctypes.c_double * 4)(*THRESHOLDS)
    _lib.check(lib.cpd_waymo_match(P(iou), P(d_pair), P(d_po), P(d_go), len(problems), sum(n_pd), sum(n_gt), P(score), P(diff),
                                   P(ph), P(gh), thr, max(n_pd), max(n_gt), 0, P(counts), P(ha), P(ws), ws_bytes,
                                   _lib.stream()), "cpd_waymo_match")
    return counts.cpu().numpy(), ha.cpu().numpy()


def ref_match(problems):
    counts, ha = np.zeros((4, 2, 101, 3), np.int64), np.zeros((4, 2, 101))
    for q, (iou, score, diff, ph, gh) in enumerate(problems):
        order = np.argsort(-np.asarray(score, np.float32).astype(np.float64), kind="stable")
        c, h = R.problem_counts(np.asarray(iou, np.float64).reshape(len(score), len(diff))[order], np.asarray(score)[order],
                                np.asarray(diff), np.asarray(ph)[order], np.asarray(gh), THRESHOLDS[q % 4])
        counts[q % 4] += c
        ha[q % 4] += h
    return counts, ha


# ---- IoU ------------------------------------------------------------------------------------------------------------

def test_iou_closed_forms_and_reference_pairs(we, wz):
    for key in ("ana", "ref"):
        a, b, want = wz[key + "_a"], wz[key + "_b"], wz[key + "_iou"]
        got = np.array([blk[0, 0] for blk in gpu_iou_blocks([x[None] for x in a], [y[None] for y in b])])
        for i in np.argsort(-np.abs(got - want))[:3]:
            print("%s pair %d: got %.12g want %.12g" % (key, i, got[i], want[i]))
        assert np.abs(got - want).max() <= 1e-7, key
    assert len(wz["ref_iou"]) >= 150 and np.count_nonzero(wz["ref_iou"] > 0.3) >= 50


def random_boxes(rng, n, centre=(20.0, -35.0), spread=6.0):
    out = np.zeros((n, 7), np.float32)
    out[:, 0] = centre[0] + rng.uniform(-spread, spread, n)
    out[:, 1] = centre[1] + rng.uniform(-spread, spread, n)
    out[:, 2] = rng.uniform(-1, 1, n)
    out[:, 3] = rng.uniform(0.3, 6.0, n)
    out[:, 4] = rng.uniform(0.3, 2.5, n)
    out[:, 5] = rng.uniform(0.5, 2.5, n)
    out[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, n)
    return out


IOU_SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 63), (257, 3)]


def test_iou_blocks_vs_restatement(we):
    rng = np.random.default_rng(5)
    pd_sets = [random_boxes(rng, r) for r, _ in IOU_SHAPES]
    gt_sets = [random_boxes(rng, c) for _, c in IOU_SHAPES]
    pd_sets[2][0] = gt_sets[2][0] + np.array([0.2, 0.1, 0.1, 0, 0, 0, 0.1], np.float32)      # the 1 x 1 block overlaps
    got = gpu_iou_blocks(pd_sets, gt_sets)          # one call: the segment offsets are exercised
    overlapping = 0
    for (r, c), p, g, blk in zip(IOU_SHAPES, pd_sets, gt_sets, got):
        assert blk.shape == (r, c)
        want = R.iou_matrix(p, g)
        overlapping += int(np.count_nonzero(want > 0))
        err = np.abs(blk - want).max(initial=0)
        print("block %d x %d: max |diff| %.3g" % (r, c, err))
        assert err <= 1e-7, (r, c)
    assert overlapping >= 500


def test_iou_degenerate_inputs_are_finite(we):
    base = np.array([3.0, 4.0, 0.5, 4.0, 2.0, 1.5, 0.3], np.float32)
    pds, want = [], []
    near = base.copy()
    near[6] = np.float32(0.3) + np.float32(1e-7)                      # nearly parallel edges
    pds.append(near), want.append(R.iou_pair(near, base))
    for col in range(7):                                             # NaN / inf anywhere gives 0
        for v in (np.nan, np.inf):
            b = base.copy()
            b[col] = v
            pds.append(b), want.append(0.0)
    zero = base.copy()
    zero[3] = 0.0                                                    # a box without volume
    pds.append(zero), want.append(0.0)
    got = gpu_iou_blocks([np.array(pds)], [base[None]])[0][:, 0]
    assert np.all(np.isfinite(got))
    assert np.abs(got - np.array(want)).max() <= 1e-7
    assert got[0] > 0.999
    back = gpu_iou_blocks([base[None]], [np.array(pds)])[0][0]        # and as the column box
    assert np.all(np.isfinite(back)) and np.abs(back - np.array(want)).max() <= 1e-7


# ---- the matching kernel alone --------------------------------------------------------------------------------------

def sparse_problem(rng, r, c, thr, density, scores="random", dense_above=False):
    iou = rng.uniform(0.05, 0.999, (r, c))
    if dense_above:
        iou = rng.uniform(thr + 0.01, 0.999, (r, c))
    else:
        iou = np.where(rng.uniform(size=(r, c)) < density, iou, rng.uniform(0, 0.2, (r, c)) * (rng.uniform(size=(r, c)) < 0.5))
        iou = np.where(np.abs(iou - thr) < 1e-4, 0.0, iou)
    if scores == "random":
        score = rng.uniform(0, 1, r).astype(np.float32)
    elif scores == "equal":
        score = np.full(r, 0.37, np.float32)
    else:                                                             # exactly on cut-offs, with repeats
        score = R.CUTOFFS[rng.integers(0, 101, r)]
    diff = rng.choice([1, 2], c).astype(np.uint8)
    return iou, score, diff, rng.uniform(-np.pi, np.pi, r).astype(np.float32), rng.uniform(-np.pi, np.pi, c).astype(np.float32)


def subset_matchings(w, score):
    out, prev = [], None
    for k in range(101):
        idx = np.nonzero(score >= R.CUTOFFS[k])[0]
        if prev is not None and len(idx) == prev:
            continue
        prev = len(idx)
        out.append(frozenset((int(idx[i]), j) for i, j in R.optimal_pairs(w[idx])))
    return out


def assert_stable(problems, rng):
    """The maker's input condition, on the CPU: no weight within 1e-4 of the threshold, and every cut-off's optimal
    matching unchanged under five random +-1e-7 perturbations -- so the expected counts do not hang on a tie."""
    for q, (iou, score, *_) in enumerate(problems):
        thr = THRESHOLDS[q % 4]
        iou = np.nan_to_num(np.asarray(iou, np.float64), nan=0.0, posinf=0.0)
        if iou.size == 0:
            continue
        assert np.abs(iou - thr).min() >= 1e-4
        w = np.where(iou >= thr, iou, 0.0)
        base = subset_matchings(w, np.asarray(score, np.float32))
        for _ in range(5):
            wp = np.where(w > 0, w + rng.uniform(-1e-7, 1e-7, w.shape), 0.0)
            assert subset_matchings(wp, np.asarray(score, np.float32)) == base, "problem %d has a near-tie" % q


def chain_problem(n, thr):
    """Rows 0..n-1 prefer column i and can move to i + 1; the last, lowest-scored row reaches only column 0, and taking
    it moves every earlier row one column on: an augmenting path through all n + 1 rows."""
    iou = np.zeros((n + 1, n + 1))
    for i in range(n):
        iou[i, i] = 0.95 - 0.01 * i
        iou[i, i + 1] = 0.93 - 0.01 * i
    iou[n, 0] = thr + 0.15
    score = np.linspace(0.9, 0.2, n + 1).astype(np.float32)
    diff = np.array([1, 2] * n, np.uint8)[:n + 1]
    heads = np.linspace(-3, 3, n + 1).astype(np.float32)
    return iou, score, diff, heads, heads[::-1].copy()


def check_match(problems, seed=0):
    assert_stable(problems, np.random.default_rng(1000 + seed))
    counts, ha = gpu_match(problems)
    want_c, want_h = ref_match(problems)
    bad = np.argwhere(counts != want_c)
    for b in bad[:5]:
        print("counts%s: got %d want %d" % (tuple(b), counts[tuple(b)], want_c[tuple(b)]))
    print("max |ha diff| %.3g" % np.abs(ha - want_h).max())
    np.testing.assert_array_equal(counts, want_c)
    assert np.all(np.abs(ha - want_h) <= 1e-9 * (1 + np.abs(want_h)))
    return counts, ha


@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (65, 63), (130, 40), (40, 130)])
def test_match_random_sparse_blocks(we, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    r, c = shape
    problems = [sparse_problem(rng, r, c, THRESHOLDS[q], 4.0 / min(r, c), dense_above=(r == 1)) for q in range(4)]
    counts, _ = check_match(problems, seed=r)
    assert counts[:, 1, 0, 0].sum() > 0                                # something matched


def test_match_dense_block_long_paths(we):
    rng = np.random.default_rng(64)
    problems = [sparse_problem(rng, 64, 64, THRESHOLDS[q], 1.0, dense_above=True) for q in range(4)]
    counts, _ = check_match(problems, seed=64)
    np.testing.assert_array_equal(counts[:, 1, 0, 0], [64] * 4)        # every column is taken at the lowest cut-off
    # greedy by score gives other pairs here: matching row by row without re-routing cannot pass
    greedy = 0
    for q, (iou, score, diff, ph, gh) in enumerate(problems):
        order = np.argsort(-score.astype(np.float64), kind="stable")
        args = (iou[order], score[order], diff, ph[order], gh, THRESHOLDS[q])
        greedy += int(not np.array_equal(R.problem_counts(*args, R.greedy_pairs)[1], R.problem_counts(*args)[1]))
    assert greedy >= 1


def test_match_all_zero_block_and_empty_problems(we):
    rng = np.random.default_rng(2)
    zero = list(sparse_problem(rng, 9, 7, 0.7, 0.5))
    zero[0] = np.zeros((9, 7))
    no_pd = (np.zeros((0, 5)), np.zeros(0, np.float32), np.array([1, 2, 1, 1, 2], np.uint8), np.zeros(0, np.float32),
             np.zeros(5, np.float32))
    no_gt = (np.zeros((6, 0)), rng.uniform(0, 1, 6).astype(np.float32), np.zeros(0, np.uint8), np.zeros(6, np.float32),
             np.zeros(0, np.float32))
    nan = list(sparse_problem(rng, 12, 10, 0.5, 0.4))
    nan[0] = nan[0].copy()
    nan[0][::3, ::2] = np.nan                                          # NaN cells count as 0
    nan[0][1, 1] = np.inf                                              # so do infinite ones
    counts, ha = check_match([tuple(zero), no_pd, no_gt, tuple(nan)])
    assert counts[0, :, :, 0].sum() == 0 and counts[0, 1, 0, 1] == 9 and counts[0, 1, 0, 2] == 7
    assert counts[1, :, :, 1].sum() == 0 and np.all(counts[1, 1, :, 2] == 5) and np.all(counts[1, 0, :, 2] == 3)
    assert counts[2, 1, 0, 1] == 6 and counts[2, :, :, 2].sum() == 0
    assert np.all(np.isfinite(ha))


@pytest.mark.parametrize("scores", ["equal", "cutoffs"])
def test_match_score_ties_and_cutoff_scores(we, scores):
    rng = np.random.default_rng(7 if scores == "equal" else 8)
    problems = [sparse_problem(rng, 40, 30, THRESHOLDS[q], 0.15, scores=scores) for q in range(4)]
    counts, _ = check_match(problems, seed=3)
    if scores == "equal":                                             # one subset: cut-offs 0..37 see it, the rest nothing
        assert np.all(counts[:, 1, :38, 0] == counts[:, 1, :1, 0]) and counts[:, :, 38:, :2].sum() == 0
        assert counts[:, 1, 0, 0].sum() > 0
    else:                                                             # a score equal to c_k belongs to subset k
        for q, p in enumerate(problems):
            for k in (0, 17, 50, 100):
                n_k = int(np.count_nonzero(p[1] >= R.CUTOFFS[k]))
                assert counts[q, 1, k, 0] + counts[q, 1, k, 1] == n_k


def test_match_chains(we):
    problems = [chain_problem(n, THRESHOLDS[q]) for q, n in enumerate((3, 5, 8, 12))]
    for q, (iou, score, *_) in enumerate(problems):                    # the last row re-routes every earlier one
        w = np.where(iou >= THRESHOLDS[q], iou, 0.0)
        before, after = dict(R.optimal_pairs(w[:-1])), dict(R.optimal_pairs(w))
        assert sum(1 for r in before if after.get(r) != before[r]) >= 3
    counts, _ = check_match(problems, seed=5)
    for q, n in enumerate((3, 5, 8, 12)):
        assert counts[q, 1, 0, 0] == n + 1 and counts[q, 1, 0, 1] == 0


# ---- end to end -----------------------------------------------------------------------------------------------------

def worked_infos():
    gt = {"name": np.array(["Vehicle", "Vehicle"]), "difficulty": np.array([0, 0]), "num_points_in_gt": np.array([50, 80]),
          "gt_boxes_lidar": np.array([[10.0, 5.0, 1.0, 4.5, 2.0, 1.6, 0.1], [-20.0, 8.0, 1.0, 4.5, 2.0, 1.6, 1.2]])}
    pd = {"name": np.array(["Vehicle"] * 3), "score": np.array([0.9, 0.8, 0.7], np.float32),
          "boxes_lidar": np.array([[10.1, 5.0, 1.0, 4.5, 2.0, 1.6, 0.1], [40.0, -30.0, 1.0, 4.5, 2.0, 1.6, 0.0],
                                   [-20.0, 8.1, 1.0, 4.5, 2.0, 1.6, 1.2]])}
    return [pd], [gt]


def test_worked_case_end_to_end(we):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    pd_infos, gt_infos = worked_infos()
    detail = {}
    got = est.waymo_evaluation(pd_infos, gt_infos, ["Vehicle", "Pedestrian", "Cyclist"], fake_gt_infos=False, detail=detail)
    assert abs(got["OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/AP"][0] - (0.5 + 0.5 * 2 / 3)) <= 1e-12
    assert abs(got["OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/AP"][0] - (0.5 + 0.5 * 2 / 3)) <= 1e-12
    for k, v in got.items():
        if "VEHICLE" not in k:
            assert v == [0.0], k
    c = detail["counts"][0, 0]
    np.testing.assert_array_equal(c[70], [2, 1, 0])
    np.testing.assert_array_equal(c[71], [1, 1, 1])
    np.testing.assert_array_equal(c[81], [1, 0, 1])
    np.testing.assert_array_equal(c[91], [0, 0, 2])


@pytest.fixture(scope="module")
def golden_run(we, wz):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    detail = {}
    classes = [str(c) for c in wz["class_names"]]
    result = est.waymo_evaluation(*R.infos_from_flat(wz), classes, detail=detail)
    return est, classes, result, detail


def test_scene_set_vs_golden(we, wz, golden_run):
    _, _, result, detail = golden_run
    assert detail["counts"].dtype == np.int64 and detail["counts"].shape == (4, 2, 101, 3)
    for b in np.argwhere(detail["counts"] != wz["counts"])[:5]:
        print("counts%s: got %d want %d" % (tuple(b), detail["counts"][tuple(b)], wz["counts"][tuple(b)]))
    np.testing.assert_array_equal(detail["counts"], wz["counts"])
    assert np.all(np.abs(detail["ha"] - wz["ha"]) <= 1e-9 * (1 + np.abs(wz["ha"])))
    assert list(result) == [str(k) for k in wz["keys"]]
    for (k, v), want in zip(result.items(), wz["values"]):
        assert isinstance(v, list) and len(v) == 1 and type(v[0]) is float
        print("%s: got %.15g want %.15g" % (k, v[0], want))
        assert abs(v[0] - want) <= 1e-12, k


def test_scene_set_in_chunks_is_identical(we, wz, golden_run):
    est, classes, result, detail = golden_run
    chunked = {}
    again = est.waymo_evaluation(*R.infos_from_flat(wz), classes, detail=chunked, chunk_frames=7)
    np.testing.assert_array_equal(chunked["counts"], detail["counts"])
    assert chunked["ha"].tobytes() == detail["ha"].tobytes()
    assert again == result


def test_raw_scores_above_one_go_through_the_sigmoid(we, wz, capsys):
    est = we.OpenPCDetWaymoDetectionMetricsEstimator()
    classes = [str(c) for c in wz["class_names"]]
    pd_infos, gt_infos = R.infos_from_flat(wz, "lg_")
    assert max(float(i["score"].max()) for i in pd_infos if len(i["score"])) > 1
    detail = {}
    got = est.waymo_evaluation(pd_infos, gt_infos, classes, detail=detail)
    assert "Warning: Waymo evaluation only supports normalized scores" in capsys.readouterr().out
    want, counts, ha = R.waymo_evaluation(*R.infos_from_flat(wz, "lg_"), classes)
    np.testing.assert_array_equal(detail["counts"], counts)
    assert list(got) == list(want)
    for k in want:
        assert abs(got[k][0] - want[k][0]) <= 1e-12, k
    assert got["OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/AP"][0] > 0
