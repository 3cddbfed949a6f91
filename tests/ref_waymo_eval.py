"""Independent numpy / scipy restatement of the Waymo-protocol detection metrics that cpd_amd.waymo_eval computes on
the GPU. It shares no code with the product: a world-frame Sutherland-Hodgman polygon clip in float64 for the IoU, a
matching from scratch at every score cut-off with scipy.optimize.linear_sum_assignment, the counts, AP / APH, and the
host preprocessing of cpd/datasets/waymo_unsupervised/waymo_eval.py (l.26-84, 169-216). Slow on purpose; tests keep it
to small sets. The protocol is the one stated in cpd_amd/waymo_eval.py's docstring; like the product it does not claim to
be the official tool."""
import copy
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

WAYMO_CLASSES = ['unknown', 'Vehicle', 'Pedestrian', 'Truck', 'Cyclist']
TYPE_NAMES = {1: 'VEHICLE', 2: 'PEDESTRIAN', 3: 'SIGN', 4: 'CYCLIST'}
IOU_THRESHOLDS = {1: 0.7, 2: 0.5, 3: 0.5, 4: 0.5}
CUTOFFS = np.array([np.float32(k * 0.01) for k in range(100)] + [np.float32(1.0)], dtype=np.float32)


# ---- IoU ------------------------------------------------------------------------------------------------------------

def corners_bev(box):
    """Counter-clockwise BEV corners [4, 2] of (cx, cy, cz, dx, dy, dz, heading), dx along the heading."""
    cx, cy, _, dx, dy, _, h = [float(v) for v in box]
    c, s = math.cos(h), math.sin(h)
    out = []
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        ex, ey = sx * dx / 2, sy * dy / 2
        out.append((cx + c * ex - s * ey, cy + s * ex + c * ey))
    return out


def _clip(subject, clip):
    """Sutherland-Hodgman: the part of polygon `subject` inside the convex counter-clockwise polygon `clip`."""
    out = list(subject)
    for i in range(len(clip)):
        ax, ay = clip[i]
        bx, by = clip[(i + 1) % len(clip)]
        src, out = out, []
        if not src:
            break

        def side(p):
            return (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)
        for k in range(len(src)):
            p, q = src[k], src[(k + 1) % len(src)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def _area(poly):
    if len(poly) < 3:
        return 0.0
    return 0.5 * abs(sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1]
                         for i in range(len(poly))))


def iou_pair(a, b):
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return 0.0
    h = min(a[2] + a[5] / 2, b[2] + b[5] / 2) - max(a[2] - a[5] / 2, b[2] - b[5] / 2)
    if not h > 0:
        return 0.0
    if a[3] <= 0 or a[4] <= 0 or b[3] <= 0 or b[4] <= 0:
        return 0.0
    if math.hypot(a[0] - b[0], a[1] - b[1]) > 0.5 * (math.hypot(a[3], a[4]) + math.hypot(b[3], b[4])) + 1e-9:
        return 0.0
    inter = _area(_clip(corners_bev(a), corners_bev(b))) * h
    union = a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter
    if not inter > 0 or not union > 0:
        return 0.0
    return inter / union


def iou_matrix(pd, gt):
    out = np.zeros((len(pd), len(gt)), dtype=np.float64)
    for i in range(len(pd)):
        for j in range(len(gt)):
            out[i, j] = iou_pair(pd[i], gt[j])
    return out


# ---- matching and counts --------------------------------------------------------------------------------------------

def heading_accuracy(pd_heading, gt_heading):
    d = float(np.float32(pd_heading)) - float(np.float32(gt_heading))
    d = (d + math.pi) % (2 * math.pi) - math.pi
    return 1.0 - abs(d) / math.pi


def optimal_pairs(weights):
    """Maximum-weight matching over the positive cells of `weights` (zero cells cannot match): list of (row, col)."""
    if weights.size == 0:
        return []
    rows, cols = linear_sum_assignment(weights, maximize=True)
    return [(int(r), int(c)) for r, c in zip(rows, cols) if weights[r, c] > 0]


def problem_counts(iou, score, difficulty, pd_heading, gt_heading, thr, pairs_fn=optimal_pairs):
    """counts [2 levels][101][tp, fp, fn] int64 and ha [2][101] float64 of one (frame, type) problem; the matching is
    solved from scratch at every cut-off whose subset differs from the previous one."""
    iou = np.nan_to_num(np.asarray(iou, dtype=np.float64).reshape(len(score), len(difficulty)), nan=0.0, posinf=0.0)
    score = np.asarray(score, dtype=np.float32)
    difficulty = np.asarray(difficulty)
    w = np.where(iou >= thr, iou, 0.0)
    level = [difficulty == 1, (difficulty == 1) | (difficulty == 2)]
    counts = np.zeros((2, 101, 3), dtype=np.int64)
    ha = np.zeros((2, 101), dtype=np.float64)
    prev, prev_key = None, None
    for k in range(101):
        idx = np.nonzero(score >= CUTOFFS[k])[0]
        key = idx.tobytes()
        if key != prev_key:
            pairs = [(int(idx[r]), c) for r, c in pairs_fn(w[idx])]
            prev_key = key
            matched_gt = np.zeros(len(difficulty), dtype=bool)
            terms = np.zeros(len(difficulty))
            for r, c in pairs:
                matched_gt[c] = True
                terms[c] = heading_accuracy(pd_heading[r], gt_heading[c])
            prev = []
            for lv in range(2):
                tp = int(np.count_nonzero(matched_gt & level[lv]))
                fn = int(np.count_nonzero(~matched_gt & level[lv]))
                fp = len(idx) - len(pairs)
                prev.append((tp, fp, fn, float(sum(terms[c] for c in range(len(difficulty)) if matched_gt[c] and level[lv][c]))))
        for lv in range(2):
            counts[lv, k] = prev[lv][:3]
            ha[lv, k] = prev[lv][3]
    return counts, ha


def greedy_pairs(weights):
    """Greedy by row order (the rows arrive sorted by descending score): each row takes its best free column."""
    taken, pairs = set(), []
    for r in range(weights.shape[0]):
        best, bc = 0.0, -1
        for c in range(weights.shape[1]):
            if c not in taken and weights[r, c] > best:
                best, bc = weights[r, c], c
        if bc >= 0:
            taken.add(bc)
            pairs.append((r, bc))
    return pairs


# ---- AP -------------------------------------------------------------------------------------------------------------

def average_precision(tp, fp, fn, ha=None):
    tp, fp, fn = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn))
    num = tp if ha is None else np.asarray(ha, dtype=np.float64)
    points = []
    for k in range(len(tp)):
        p = num[k] / (tp[k] + fp[k]) if tp[k] + fp[k] > 0 else 0.0
        r = num[k] / (tp[k] + fn[k]) if tp[k] + fn[k] > 0 else 0.0
        points.append((r, p))
    recalls = sorted({r for r, _ in points if r > 0})
    ap, last = 0.0, 0.0
    for rho in recalls:
        ap += (rho - last) * max(p for r, p in points if r >= rho)
        last = rho
    return float(ap)


def result_dict(counts, ha):
    """counts [4][2][101][3], ha [4][2][101] -> the estimator's dict, in its key order."""
    out = {}
    for t in (1, 2, 3, 4):
        for lv in (1, 2):
            c = counts[t - 1, lv - 1]
            stem = 'OBJECT_TYPE_TYPE_%s_LEVEL_%d/' % (TYPE_NAMES[t], lv)
            out[stem + 'AP'] = [average_precision(c[:, 0], c[:, 1], c[:, 2])]
            out[stem + 'APH'] = [average_precision(c[:, 0], c[:, 1], c[:, 2], ha[t - 1, lv - 1])]
    return out


# ---- host preprocessing (waymo_eval.py:19-84, 169-216) --------------------------------------------------------------

def limit_period(val, offset=0.5, period=np.pi):
    return val - np.floor(val / period + offset) * period


def generate_waymo_type_results(infos, class_names, is_gt=False, fake_gt_infos=True):
    infos = copy.deepcopy(infos)
    frame_id, boxes3d, obj_type, score, overlap_nlz, difficulty = [], [], [], [], [], []
    for frame_index, info in enumerate(infos):
        if is_gt:
            box_mask = np.array([n in class_names for n in info['name']], dtype=np.bool_)
            if 'num_points_in_gt' not in info:
                raise NotImplementedError
            zero = info['difficulty'] == 0
            info['difficulty'][(info['num_points_in_gt'] > 5) & zero] = 1
            info['difficulty'][(info['num_points_in_gt'] <= 5) & zero] = 2
            box_mask = box_mask & (info['num_points_in_gt'] > 0)
            num_boxes = box_mask.sum()
            box_name = info['name'][box_mask]
            difficulty.append(info['difficulty'][box_mask])
            score.append(np.ones(num_boxes))
            if fake_gt_infos:
                b = info['gt_boxes_lidar']
                w, l, h, r = b[:, 3:4], b[:, 4:5], b[:, 5:6], b[:, 6:7]
                b[:, 2] += h[:, 0] / 2
                info['gt_boxes_lidar'] = np.concatenate([b[:, 0:3], l, w, h, -(r + np.pi / 2)], axis=-1)
            boxes3d.append(info['gt_boxes_lidar'][box_mask])
        else:
            num_boxes = len(info['boxes_lidar'])
            difficulty.append([0] * num_boxes)
            score.append(info['score'])
            boxes3d.append(np.array(info['boxes_lidar']))
            box_name = info['name']
        obj_type += [WAYMO_CLASSES.index(name) for name in box_name]
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


def mask_by_distance(distance_thresh, boxes_3d, *args):
    mask = np.linalg.norm(boxes_3d[:, 0:2], axis=1) < distance_thresh + 0.5
    return (boxes_3d[mask],) + tuple(arg[mask] for arg in args)


def problems(pd_frame, pd_boxes, pd_type, pd_score, gt_frame, gt_boxes, gt_type, gt_difficulty, n_frames):
    """Yield (frame, type, pd index array, gt index array) for every (frame, type) in order."""
    for f in range(n_frames):
        for t in (1, 2, 3, 4):
            yield f, t, np.nonzero((pd_frame == f) & (pd_type == t))[0], np.nonzero((gt_frame == f) & (gt_type == t))[0]


def evaluate_arrays(pd_frame, pd_boxes, pd_type, pd_score, gt_frame, gt_boxes, gt_type, gt_difficulty, n_frames,
                    pairs_fn=optimal_pairs):
    """counts [4][2][101][3] int64, ha [4][2][101] float64 and the per-problem IoU blocks, from the op's inputs."""
    pd_boxes = np.asarray(pd_boxes, dtype=np.float32)
    gt_boxes = np.asarray(gt_boxes, dtype=np.float32)
    pd_score = np.asarray(pd_score, dtype=np.float32)
    counts = np.zeros((4, 2, 101, 3), dtype=np.int64)
    ha = np.zeros((4, 2, 101), dtype=np.float64)
    blocks = []
    for f, t, pi, gi in problems(pd_frame, pd_boxes, pd_type, pd_score, gt_frame, gt_boxes, gt_type, gt_difficulty,
                                 n_frames):
        order = pi[np.argsort(-pd_score[pi].astype(np.float64), kind='stable')]
        iou = iou_matrix(pd_boxes[order], gt_boxes[gi])
        c, h = problem_counts(iou, pd_score[order], gt_difficulty[gi], pd_boxes[order, 6], gt_boxes[gi, 6],
                              IOU_THRESHOLDS[t], pairs_fn)
        counts[t - 1] += c
        ha[t - 1] += h
        blocks.append((f, t, order, gi, iou))
    return counts, ha, blocks


def waymo_evaluation(prediction_infos, gt_infos, class_name, distance_thresh=100, fake_gt_infos=True):
    assert len(prediction_infos) == len(gt_infos)
    pd_frame, pd_boxes, pd_type, pd_score, pd_nlz, _ = generate_waymo_type_results(prediction_infos, class_name, False)
    gt_frame, gt_boxes, gt_type, gt_score, _, gt_diff = generate_waymo_type_results(gt_infos, class_name, True,
                                                                                   fake_gt_infos)
    pd_boxes, pd_frame, pd_type, pd_score, pd_nlz = mask_by_distance(distance_thresh, pd_boxes, pd_frame, pd_type,
                                                                     pd_score, pd_nlz)
    gt_boxes, gt_frame, gt_type, gt_score, gt_diff = mask_by_distance(distance_thresh, gt_boxes, gt_frame, gt_type,
                                                                      gt_score, gt_diff)
    if len(pd_score) and pd_score.max() > 1:
        pd_score = 1 / (1 + np.exp(-pd_score))
    counts, ha, _ = evaluate_arrays(pd_frame, pd_boxes, pd_type, pd_score, gt_frame, gt_boxes, gt_type, gt_diff,
                                    len(gt_infos))
    return result_dict(counts, ha), counts, ha


# ---- infos <-> flat arrays (golden storage) -------------------------------------------------------------------------

def infos_to_flat(pd_infos, gt_infos, prefix=""):
    cat = lambda parts, tail, dtype: (np.concatenate([np.asarray(p, dtype=dtype).reshape((-1,) + tail) for p in parts], 0)
                                      if parts else np.zeros((0,) + tail, dtype))
    return {
        prefix + "pd_num": np.array([len(i["name"]) for i in pd_infos], np.int64),
        prefix + "pd_boxes": cat([i["boxes_lidar"] for i in pd_infos], (7,), np.float32),
        prefix + "pd_score": cat([i["score"] for i in pd_infos], (), np.float32),
        prefix + "pd_name": np.concatenate([np.asarray(i["name"], dtype="<U16") for i in pd_infos]),
        prefix + "gt_num": np.array([len(i["name"]) for i in gt_infos], np.int64),
        prefix + "gt_boxes": cat([i["gt_boxes_lidar"] for i in gt_infos], (7,), np.float32),
        prefix + "gt_name": np.concatenate([np.asarray(i["name"], dtype="<U16") for i in gt_infos]),
        prefix + "gt_difficulty": cat([i["difficulty"] for i in gt_infos], (), np.int32),
        prefix + "gt_points": cat([i["num_points_in_gt"] for i in gt_infos], (), np.int64),
    }


def infos_from_flat(z, prefix=""):
    """(prediction_infos, gt_infos) as Dataset.evaluation passes them: fresh arrays on every call."""
    pd_off = np.concatenate([[0], np.cumsum(z[prefix + "pd_num"])])
    gt_off = np.concatenate([[0], np.cumsum(z[prefix + "gt_num"])])
    pd_infos, gt_infos = [], []
    for f in range(len(pd_off) - 1):
        s = slice(pd_off[f], pd_off[f + 1])
        pd_infos.append({"name": np.array(z[prefix + "pd_name"][s]), "score": np.array(z[prefix + "pd_score"][s]),
                         "boxes_lidar": np.array(z[prefix + "pd_boxes"][s])})
        s = slice(gt_off[f], gt_off[f + 1])
        gt_infos.append({"name": np.array(z[prefix + "gt_name"][s]), "difficulty": np.array(z[prefix + "gt_difficulty"][s]),
                         "num_points_in_gt": np.array(z[prefix + "gt_points"][s]),
                         "gt_boxes_lidar": np.array(z[prefix + "gt_boxes"][s])})
    return pd_infos, gt_infos
