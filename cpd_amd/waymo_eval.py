"""Waymo-protocol detection metrics (L1 / L2 AP and APH per object type) on the GPU: a drop-in for
cpd/datasets/waymo_unsupervised/waymo_eval.py with no tensorflow / waymo_open_dataset dependency.

Same public surface: OpenPCDetWaymoDetectionMetricsEstimator (a plain class here) with generate_waymo_type_results,
mask_by_distance, build_config and waymo_evaluation(prediction_infos, gt_infos, class_name, distance_thresh=100,
fake_gt_infos=True) -> {'OBJECT_TYPE_TYPE_<T>_LEVEL_<L>/AP' | '/APH': [float]}, in the order VEHICLE, PEDESTRIAN, SIGN,
CYCLIST x LEVEL_1, LEVEL_2 x AP, APH. The reference's caller reads ap_dict[key][0].

PARITY STATUS. The metric itself is implemented inside waymo_open_dataset, not in the reference tree; it was neither run
nor read when this module was written. What is computed here is the published definition -- the reference's metric config
(waymo_eval.py:86-108) and the AP / APH formulas of the Waymo Open Dataset paper (Sun et al., CVPR 2020, section 5.1) --
restated as the protocol below. No bit-parity with the official tool is claimed. Known unknowns:
  * Recall interpolation. The official AP routine takes a max_recall_delta and is believed to insert interpolated points
    where neighbouring operating points lie more than 0.05 apart in recall. That is not reproduced; values can differ
    from the official tool's where the PR curve has such gaps.
  * Tie handling. The official Hungarian matcher may quantise IoU to integers before matching. Here the weights are
    float64; when two matchings of a problem tie, or nearly tie, in total IoU, the choice may differ.
  * IoU near a threshold. The official IoU comes from its own polygon code; pairs within rounding of a threshold can
    fall on the other side.
  * APL. Later library versions also emit '/APL'. It is not produced here.

PROTOCOL. Type ids 1..4 (WAYMO_CLASSES index; id 3, 'Truck', lands in the SIGN breakdown as in the reference) have IoU
thresholds 0.7, 0.5, 0.5, 0.5. Cut-offs are c_k = float32(k * 0.01) for k = 0..99 and c_100 = 1.0; a prediction with
float32 score s belongs to subset k iff s >= c_k.
  IoU: boxes are float32 rows (cx, cy, cz, dx, dy, dz, heading), dx along the heading; arithmetic is float64. IoU = (area
of the intersection of the two rotated BEV rectangles x overlap of the z intervals [cz +- dz/2]) / (vol_a + vol_b - that);
0 when the intersection is empty or the union is not positive; a NaN anywhere gives 0.
  Matching: per frame, type and cut-off k, over the predictions of subset k and the ground truths of every difficulty of
that frame and type: the matching that maximises the sum of IoU over pairs with IoU >= the type's threshold (pairs below
it cannot match).
  Counts: a ground truth counts at level 1 iff its difficulty is 1, at level 2 iff it is 1 or 2. TP_L = matched ground
truths that count at L, FN_L = unmatched ones, FP = unmatched predictions of subset k (the same for both levels: a
prediction matched to a ground truth that does not count at L is neither TP nor FP at L), HA_L = sum over TP_L of
1 - |wrap(heading_pd - heading_gt)| / pi with wrap to [-pi, pi]. Counts are summed over frames in frame order.
  AP: p_k = tp / (tp + fp) (0 if the denominator is 0), r_k = tp / (tp + fn) (0 without ground truths);
AP = sum_i (rho_i - rho_{i-1}) * max{p_j : r_j >= rho_i} over the distinct positive recalls rho_1 < rho_2 < ..., rho_0 = 0:
the paper's integral of max{p(r') | r' >= r} dr evaluated exactly on the 101 operating points. APH is the same with
ha / (tp + fp) and ha / (tp + fn).

WHERE THE WORK RUNS. The class / difficulty / distance masks, the fake-lidar conversion and the AP integration stay on the
host (numpy, float64). Frames go to the GPU in chunks whose packed pair count stays under PAIR_BUDGET (2^27 pairs, 1 GiB of
float64 IoUs): per chunk one cpd_waymo_iou launch (every (frame, type) block) and one cpd_waymo_match launch (every problem's
101 matchings by one incremental assignment solve, then the frame-order reduction). The running totals stay on the device
between chunks, so the heading sums add the same terms in the same order however the frames are chunked, and are read back
once. There is no per-frame Python loop. Limits: at most CPD_WAYMO_MAX_PD = 4096 predictions and CPD_WAYMO_MAX_GT = 1024
ground truths per (frame, type); beyond them CpdHipError (CPD_ERR_UNSUPPORTED). No GPU raises CpdHipError: there is no
CPU fallback.

OTHER BOX TYPE, OTHER THRESHOLDS. evaluate_arrays(..., box_type='TYPE_2D') is the BEV protocol of waymo_eval2d.py (rows
(cx, cy, dx, dy, heading), cpd_waymo_iou_bev, own thresholds 0.5 / 0.3 / 0.3 / 0.3; cpd_amd.waymo_eval2d is its drop-in).
iou_thresholds= replaces the protocol's set by one set of 4 or by a sequence of S sets; with S sets every chunk's IoU block
is still computed once and cpd_waymo_match runs once per set over it, into that set's totals (results get a leading axis
S). OpenPCDetWaymoDetectionMetricsEstimator.waymo_evaluation_at(..., iou_thresholds) returns one result dict per set, e.g.
vehicle AP at IoU 0.7 and at 0.5 from one pass. The defaults are the protocol above, bit for bit.

Differences from the reference's host code, all deliberate: generate_waymo_type_results does not modify the caller's
infos (the reference rewrites info['difficulty'] and info['gt_boxes_lidar'] in place; Dataset.evaluation passes deep
copies anyway), and a prediction set with no boxes at all evaluates to zeros where the reference's pd_score.max() raises.
"""
import numpy as np
import torch

from . import _lib

N_CUTOFFS = 101
N_TYPES = 4
IOU_THRESHOLDS = (0.7, 0.5, 0.5, 0.5)          # type ids 1..4 (build_config's iou_thresholds[1:])
# box_type -> (row width, heading column, IoU entry point, the protocol's own thresholds): waymo_eval.py and waymo_eval2d.py
BOX_TYPES = {'TYPE_3D': (7, 6, 'cpd_waymo_iou', IOU_THRESHOLDS),
             'TYPE_2D': (5, 4, 'cpd_waymo_iou_bev', (0.5, 0.3, 0.3, 0.3))}
TYPE_NAMES = ('VEHICLE', 'PEDESTRIAN', 'SIGN', 'CYCLIST')
LEVELS = (1, 2)
MAX_PD, MAX_GT = 4096, 1024                    # CPD_WAYMO_MAX_PD / CPD_WAYMO_MAX_GT
PAIR_BUDGET = 1 << 27
SCORE_CUTOFFS = np.array([np.float32(k * 0.01) for k in range(100)] + [np.float32(1.0)], dtype=np.float32)


def limit_period(val, offset=0.5, period=np.pi):
    return val - np.floor(val / period + offset) * period


def average_precision(tp, fp, fn, ha=None):
    """AP of per-cut-off counts (APH when the heading-accuracy sums `ha` are given), float64 on the host: the area under
    max{p_j : r_j >= r} for r in (0, max recall], exact on the given operating points. Returns a Python float."""
    tp, fp, fn = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (tp, fp, fn))
    if not (tp.shape == fp.shape == fn.shape):
        raise ValueError("average_precision: tp, fp and fn differ in length (%d, %d, %d)" % (tp.size, fp.size, fn.size))
    num = tp if ha is None else np.asarray(ha, dtype=np.float64).reshape(-1)
    if num.shape != tp.shape:
        raise ValueError("average_precision: ha has %d entries, the counts %d" % (num.size, tp.size))
    det, gts = tp + fp, tp + fn
    precision = np.divide(num, det, out=np.zeros_like(num), where=det > 0)
    recall = np.divide(num, gts, out=np.zeros_like(num), where=gts > 0)
    order = np.argsort(-recall, kind='stable')                     # descending recall
    r, best = recall[order], np.maximum.accumulate(precision[order])   # best[i] = max precision at recall >= r[i]
    keep = r > 0
    r, best = r[keep], best[keep]
    if r.size == 0:
        return 0.0
    last = np.append(r[1:] != r[:-1], True)                        # the last entry of each run of equal recalls
    rho, p = r[last][::-1], best[last][::-1]                       # ascending distinct recalls
    return float(np.sum((rho - np.concatenate([[0.0], rho[:-1]])) * p))


def _device():
    if not torch.cuda.is_available():
        raise _lib.CpdHipError("cpd_amd.waymo_eval needs a GPU: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_device())


def _offsets(counts, dtype):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=off[1:])
    return off.astype(dtype)


def _checked(name, frame_id, boxes, obj_type, n_frames, width=7, **per_box):
    """The op's inputs with the casts of its placeholders (float32 boxes / scores, uint8 types / difficulties)."""
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or boxes.shape[1] != width:
        raise ValueError("waymo_eval: %s boxes must be [N, %d], got %s" % (name, width, boxes.shape))
    if boxes.dtype.kind not in "fiu":
        raise TypeError("waymo_eval: %s boxes must be numeric, got %s" % (name, boxes.dtype))
    n = boxes.shape[0]
    frame_id = np.asarray(frame_id)
    obj_type = np.asarray(obj_type)
    out = {}
    for key, (arr, dtype) in dict(per_box, frame=(frame_id, np.int64), type=(obj_type, np.uint8)).items():
        arr = np.asarray(arr)
        if arr.shape != (n,):
            raise ValueError("waymo_eval: %s %s has shape %s for %d boxes" % (name, key, arr.shape, n))
        if arr.dtype.kind not in "fiub":
            raise TypeError("waymo_eval: %s %s must be numeric, got %s" % (name, key, arr.dtype))
        out[key] = arr.astype(dtype)
    if n and (out["frame"].min() < 0 or out["frame"].max() >= n_frames):
        raise ValueError("waymo_eval: %s frame ids outside 0..%d" % (name, n_frames - 1))
    out["boxes"] = boxes.astype(np.float32)
    return out


def _grouped(rec, n_frames):
    """Rows of the types 1..4 ordered by (frame, type), stable, and the row count of each of the 4 * n_frames problems."""
    keep = np.nonzero((rec["type"] >= 1) & (rec["type"] <= N_TYPES))[0]
    key = rec["frame"][keep] * N_TYPES + (rec["type"][keep].astype(np.int64) - 1)
    order = keep[np.argsort(key, kind='stable')]
    counts = np.bincount(key, minlength=N_TYPES * n_frames).astype(np.int64)
    return {k: v[order] for k, v in rec.items()}, counts


def _chunks(pairs_per_frame, chunk_frames, pair_budget):
    """Frame ranges [f0, f1): as many consecutive frames as keep the packed pair count within the budget (a frame that
    alone exceeds it goes alone), and at most chunk_frames of them."""
    n = len(pairs_per_frame)
    bounds, f0 = [], 0
    while f0 < n:
        total = np.cumsum(pairs_per_frame[f0:])
        f1 = f0 + max(1, int(np.searchsorted(total, pair_budget, side='right')))
        if chunk_frames:
            f1 = min(f1, f0 + int(chunk_frames))
        f1 = min(f1, n)
        bounds.append((f0, f1))
        f0 = f1
    return bounds


def _threshold_sets(iou_thresholds, default):
    """(the sets as a list of 4-tuples of float, whether the caller gave a sequence of sets and not one set)."""
    if iou_thresholds is None:
        iou_thresholds = default
    if iou_thresholds is None:
        raise ValueError("waymo_eval: no IoU threshold set")
    sets = list(iou_thresholds)
    stacked = bool(sets) and not np.isscalar(sets[0])
    sets = [tuple(float(v) for v in one) for one in sets] if stacked else [tuple(float(v) for v in sets)]
    if not sets:
        raise ValueError("waymo_eval: no IoU threshold set")
    for one in sets:
        if len(one) != N_TYPES:
            raise ValueError("waymo_eval: a threshold set has one value per type id 1..%d, got %d" % (N_TYPES, len(one)))
        if not all(0.0 < v <= 1.0 for v in one):
            raise ValueError("waymo_eval: IoU thresholds must lie in (0, 1], got %s" % (one,))
    return sets, stacked


def evaluate_arrays(pd_frame, pd_boxes, pd_type, pd_score, gt_frame, gt_boxes, gt_type, gt_difficulty, n_frames,
                    chunk_frames=None, pair_budget=PAIR_BUDGET, box_type='TYPE_3D', iou_thresholds=None):
    """The metric op's part: counts [4 types][2 levels][101 cut-offs][tp, fp, fn] int64 and heading-accuracy sums
    [4][2][101] float64 of the given predictions and ground truths (frame ids 0..n_frames-1, types 0..255).
    `box_type`: 'TYPE_3D' (rows [N, 7], rotated 3-D IoU) or 'TYPE_2D' (rows [N, 5] = (cx, cy, dx, dy, heading), the
    rectangles' IoU). `iou_thresholds`: None for the protocol's own set, one set of 4 (type ids 1..4), or a sequence of S
    sets -- then both results get a leading axis S; every chunk's IoU block is computed once and matched once per set."""
    if box_type not in BOX_TYPES:
        raise ValueError("waymo_eval: box_type must be one of %s, got %r" % (sorted(BOX_TYPES), box_type))
    width, heading_col, iou_entry, own_thresholds = BOX_TYPES[box_type]
    sets, stacked = _threshold_sets(iou_thresholds, own_thresholds)
    n_frames = int(n_frames)
    if n_frames < 0:
        raise ValueError("waymo_eval: n_frames is %d" % n_frames)
    pd = _checked("prediction", pd_frame, pd_boxes, pd_type, n_frames, width, score=(pd_score, np.float32))
    gt = _checked("ground-truth", gt_frame, gt_boxes, gt_type, n_frames, width, difficulty=(gt_difficulty, np.uint8))
    if np.isnan(pd["score"]).any():
        raise ValueError("waymo_eval: NaN prediction score")
    dev = _device()
    counts = torch.zeros((len(sets), N_TYPES, 2, N_CUTOFFS, 3), dtype=torch.int64, device=dev)
    ha = torch.zeros((len(sets), N_TYPES, 2, N_CUTOFFS), dtype=torch.float64, device=dev)
    if n_frames == 0:
        counts, ha = counts.cpu().numpy(), ha.cpu().numpy()
        return (counts, ha) if stacked else (counts[0], ha[0])
    pd, pd_n = _grouped(pd, n_frames)
    gt, gt_n = _grouped(gt, n_frames)
    if pd_n.max(initial=0) > MAX_PD or gt_n.max(initial=0) > MAX_GT:
        raise _lib.CpdHipError("waymo_eval: a (frame, type) holds %d predictions / %d ground truths; the limits are %d / %d "
                               "(CPD_ERR_UNSUPPORTED)" % (pd_n.max(initial=0), gt_n.max(initial=0), MAX_PD, MAX_GT))
    pd_off, gt_off = _offsets(pd_n, np.int64), _offsets(gt_n, np.int64)
    if pd_off[-1] > np.iinfo(np.int32).max or gt_off[-1] > np.iinfo(np.int32).max:
        raise _lib.CpdHipError("waymo_eval: more than 2^31 boxes")
    pairs = pd_n * gt_n
    d_pd_boxes, d_gt_boxes = _to_dev(pd["boxes"], np.float32), _to_dev(gt["boxes"], np.float32)
    d_pd_head, d_gt_head = (_to_dev(pd["boxes"][:, heading_col], np.float32),
                            _to_dev(gt["boxes"][:, heading_col], np.float32))
    d_score, d_diff = _to_dev(pd["score"], np.float32), _to_dev(gt["difficulty"], np.uint8)
    thr = [(_lib._D * N_TYPES)(*one) for one in sets]
    lib, P = _lib.lib(), _lib.ptr
    iou_fn = getattr(lib, iou_entry)
    for c, (f0, f1) in enumerate(_chunks(pairs.reshape(n_frames, N_TYPES).sum(1), chunk_frames, pair_budget)):
        q0, q1 = f0 * N_TYPES, f1 * N_TYPES
        p0, p1, g0, g1 = int(pd_off[q0]), int(pd_off[q1]), int(gt_off[q0]), int(gt_off[q1])
        pair_off = _offsets(pairs[q0:q1], np.int64)
        n_pairs = int(pair_off[-1])
        d_poff, d_goff = _to_dev(pd_off[q0:q1 + 1] - p0, np.int32), _to_dev(gt_off[q0:q1 + 1] - g0, np.int32)
        d_pair_off = _to_dev(pair_off, np.int64)
        iou = torch.empty(max(n_pairs, 1), dtype=torch.float64, device=dev)
        _lib.check(iou_fn(P(d_pd_boxes[p0:p1]), P(d_gt_boxes[g0:g1]), P(d_poff), P(d_goff), P(d_pair_off),
                          q1 - q0, n_pairs, P(iou), _lib.stream()), iou_entry)
        ws_bytes = lib.cpd_waymo_match_workspace_bytes(q1 - q0, p1 - p0)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        for s in range(len(sets)):                  # the same IoU block under every threshold set, in stream order
            _lib.check(lib.cpd_waymo_match(P(iou), P(d_pair_off), P(d_poff), P(d_goff), q1 - q0, p1 - p0, g1 - g0,
                                           P(d_score[p0:p1]), P(d_diff[g0:g1]), P(d_pd_head[p0:p1]), P(d_gt_head[g0:g1]),
                                           thr[s], int(pd_n[q0:q1].max()), int(gt_n[q0:q1].max()), int(c > 0),
                                           P(counts[s]), P(ha[s]), P(ws), ws_bytes, _lib.stream()), "cpd_waymo_match")
    counts, ha = counts.cpu().numpy(), ha.cpu().numpy()
    if counts.min() < 0:
        raise _lib.CpdHipError("cpd_waymo_match: a problem exceeded the maxima passed to it")
    return (counts, ha) if stacked else (counts[0], ha[0])


def result_dict(counts, ha):
    """The estimator's dict from counts [4][2][101][3] and ha [4][2][101], in its key order."""
    out = {}
    for t, name in enumerate(TYPE_NAMES):
        for l, level in enumerate(LEVELS):
            c = counts[t, l]
            stem = 'OBJECT_TYPE_TYPE_%s_LEVEL_%d/' % (name, level)
            out[stem + 'AP'] = [average_precision(c[:, 0], c[:, 1], c[:, 2])]
            out[stem + 'APH'] = [average_precision(c[:, 0], c[:, 1], c[:, 2], ha[t, l])]
    return out


class OpenPCDetWaymoDetectionMetricsEstimator:
    WAYMO_CLASSES = ['unknown', 'Vehicle', 'Pedestrian', 'Truck', 'Cyclist']
    BOX_TYPE = 'TYPE_3D'
    BOX_COLUMNS = None          # the columns of the seven-column boxes that the op is fed: all (waymo_eval2d: [0, 1, 3, 4, 6])

    def generate_waymo_type_results(self, infos, class_names, is_gt=False, fake_gt_infos=True):
        """(frame_id int64, boxes3d, obj_type, score, overlap_nlz, difficulty int8) of waymo_eval.py:26-84. Unlike the
        reference it leaves `infos` as it found them."""
        frame_id, boxes3d, obj_type, score, overlap_nlz, difficulty = [], [], [], [], [], []
        for frame_index, info in enumerate(infos):
            if is_gt:
                box_mask = np.array([n in class_names for n in info['name']], dtype=np.bool_)
                if 'num_points_in_gt' not in info:
                    print('Please provide the num_points_in_gt for evaluating on Waymo Dataset '
                          '(If you create Waymo Infos before 20201126, please re-create the validation infos '
                          'with version 1.2 Waymo dataset to get this attribute). SSS of OpenPCDet')
                    raise NotImplementedError
                num_points = np.asarray(info['num_points_in_gt'])
                level = np.array(info['difficulty'], copy=True)
                zero_difficulty_mask = level == 0
                level[(num_points > 5) & zero_difficulty_mask] = 1
                level[(num_points <= 5) & zero_difficulty_mask] = 2
                box_mask = box_mask & (num_points > 0)
                num_boxes = box_mask.sum()
                box_name = np.asarray(info['name'])[box_mask]
                difficulty.append(level[box_mask])
                score.append(np.ones(num_boxes))
                gt_boxes = np.array(info['gt_boxes_lidar'], copy=True)
                if fake_gt_infos:       # boxes3d_kitti_fakelidar_to_lidar: (x, y, z bottom, w, l, h, r) -> centre boxes
                    w, l, h, r = gt_boxes[:, 3:4], gt_boxes[:, 4:5], gt_boxes[:, 5:6], gt_boxes[:, 6:7]
                    gt_boxes[:, 2] += h[:, 0] / 2
                    gt_boxes = np.concatenate([gt_boxes[:, 0:3], l, w, h, -(r + np.pi / 2)], axis=-1)
                boxes = gt_boxes[box_mask]
            else:
                num_boxes = len(info['boxes_lidar'])
                difficulty.append([0] * num_boxes)
                score.append(info['score'])
                boxes = np.array(info['boxes_lidar'])
                box_name = info['name']
            boxes3d.append(boxes if self.BOX_COLUMNS is None else boxes[:, self.BOX_COLUMNS])
            obj_type += [self.WAYMO_CLASSES.index(name) for name in box_name]
            frame_id.append(np.array([frame_index] * num_boxes))
            overlap_nlz.append(np.zeros(num_boxes))
        frame_id = np.concatenate(frame_id).reshape(-1).astype(np.int64)
        boxes3d = np.concatenate(boxes3d, axis=0)
        obj_type = np.array(obj_type).reshape(-1)
        score = np.concatenate(score).reshape(-1)
        overlap_nlz = np.concatenate(overlap_nlz).reshape(-1)
        difficulty = np.concatenate(difficulty).reshape(-1).astype(np.int8)
        boxes3d[:, -1] = limit_period(boxes3d[:, -1], offset=0.5, period=np.pi * 2)
        return frame_id, boxes3d, obj_type, score, overlap_nlz, difficulty

    def build_config(self):
        """The metric config of waymo_eval.py:86-108 as a plain dict."""
        return {
            'breakdown_generator_ids': ['OBJECT_TYPE'],
            'difficulties': {'levels': list(LEVELS)},
            'matcher_type': 'TYPE_HUNGARIAN',
            'iou_thresholds': [0.0] + list(BOX_TYPES[self.BOX_TYPE][3]),
            'box_type': self.BOX_TYPE,
            'score_cutoffs': [x * 0.01 for x in range(0, 100)] + [1.0],
        }

    def mask_by_distance(self, distance_thresh, boxes_3d, *args):
        mask = np.linalg.norm(boxes_3d[:, 0:2], axis=1) < distance_thresh + 0.5
        boxes_3d = boxes_3d[mask]
        ret_ans = [boxes_3d]
        for arg in args:
            ret_ans.append(arg[mask])
        return tuple(ret_ans)

    def waymo_evaluation(self, prediction_infos, gt_infos, class_name, distance_thresh=100, fake_gt_infos=True,
                         detail=None, chunk_frames=None, pair_budget=PAIR_BUDGET):
        """waymo_eval.py:178-216. `detail`, when a dict, receives the raw per-cut-off counts: 'counts' [4][2][101][3]
        int64 (tp, fp, fn), 'ha' [4][2][101] float64 and 'score_cutoffs' [101] float32. `chunk_frames` caps the frames
        per GPU chunk and `pair_budget` its packed pairs; the result depends on neither."""
        counts, ha = self._counts(prediction_infos, gt_infos, class_name, distance_thresh, fake_gt_infos, None, detail,
                                  chunk_frames, pair_budget)
        return result_dict(counts, ha)

    def waymo_evaluation_at(self, prediction_infos, gt_infos, class_name, iou_thresholds, distance_thresh=100,
                            fake_gt_infos=True, detail=None, chunk_frames=None, pair_budget=PAIR_BUDGET):
        """waymo_evaluation under each of the given IoU threshold sets (a sequence of sets of 4, type ids 1..4; e.g.
        vehicle AP at 0.5 and at 0.7): a list of result dicts, one per set, for one pass over the IoU blocks. `detail`
        receives 'counts' [S][4][2][101][3] and 'ha' [S][4][2][101]."""
        sets, stacked = _threshold_sets(iou_thresholds, None)
        if not stacked:
            raise ValueError("waymo_eval: waymo_evaluation_at takes a sequence of threshold sets")
        counts, ha = self._counts(prediction_infos, gt_infos, class_name, distance_thresh, fake_gt_infos, sets, detail,
                                  chunk_frames, pair_budget)
        return [result_dict(c, h) for c, h in zip(counts, ha)]

    def _counts(self, prediction_infos, gt_infos, class_name, distance_thresh, fake_gt_infos, iou_thresholds, detail,
                chunk_frames, pair_budget):
        print('Start the waymo evaluation...')

        assert len(prediction_infos) == len(gt_infos), '%d vs %d' % (prediction_infos.__len__(), gt_infos.__len__())

        pd_frameid, pd_boxes3d, pd_type, pd_score, pd_overlap_nlz, _ = self.generate_waymo_type_results(
            prediction_infos, class_name, is_gt=False
        )
        gt_frameid, gt_boxes3d, gt_type, gt_score, gt_overlap_nlz, gt_difficulty = self.generate_waymo_type_results(
            gt_infos, class_name, is_gt=True, fake_gt_infos=fake_gt_infos
        )

        pd_boxes3d, pd_frameid, pd_type, pd_score, pd_overlap_nlz = self.mask_by_distance(
            distance_thresh, pd_boxes3d, pd_frameid, pd_type, pd_score, pd_overlap_nlz
        )
        gt_boxes3d, gt_frameid, gt_type, gt_score, gt_difficulty = self.mask_by_distance(
            distance_thresh, gt_boxes3d, gt_frameid, gt_type, gt_score, gt_difficulty
        )

        print('Number: (pd, %d) VS. (gt, %d)' % (len(pd_boxes3d), len(gt_boxes3d)))
        print('Level 1: %d, Level2: %d)' % ((gt_difficulty == 1).sum(), (gt_difficulty == 2).sum()))

        if len(pd_score) and pd_score.max() > 1:
            pd_score = 1 / (1 + np.exp(-pd_score))
            print('Warning: Waymo evaluation only supports normalized scores')

        counts, ha = evaluate_arrays(pd_frameid, pd_boxes3d, pd_type, pd_score, gt_frameid, gt_boxes3d, gt_type,
                                     gt_difficulty, len(gt_infos), chunk_frames=chunk_frames, pair_budget=pair_budget,
                                     box_type=self.BOX_TYPE, iou_thresholds=iou_thresholds)
        if detail is not None:
            detail['counts'], detail['ha'], detail['score_cutoffs'] = counts, ha, SCORE_CUTOFFS.copy()
        return counts, ha
