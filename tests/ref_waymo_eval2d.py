"""Independent numpy / scipy restatement of the BEV-protocol Waymo metrics that cpd_amd.waymo_eval2d computes on the GPU
(cpd/datasets/waymo_unsupervised/waymo_eval2d.py: box_type TYPE_2D, five-column boxes, IoU 0.5 / 0.3 / 0.3 / 0.3). The
polygon clip, the matching from scratch at every cut-off, the counts and the AP integration are tests/ref_waymo_eval.py's;
what is added here is the rectangle IoU without a z term, the 2-D slicing of the host preprocessing (l.26-85), and an
evaluation that takes its thresholds as a parameter. Shares no code with the product. Slow on purpose."""
import copy
import math

import numpy as np

from ref_waymo_eval import (CUTOFFS, WAYMO_CLASSES, _area, _clip, average_precision, corners_bev,  # noqa: F401
                            limit_period, mask_by_distance, optimal_pairs, problem_counts, result_dict)

IOU_THRESHOLDS = (0.5, 0.3, 0.3, 0.3)          # type ids 1..4 (waymo_eval2d.py:96-100)
VALUE_LIMIT = 2.0 ** 29                        # a row holding a magnitude at or beyond it is treated as a non-finite one

_OCT = 2.0 * (math.sqrt(2.0) - 1.0)            # a unit square and itself turned by 45 degrees share a regular octagon
# (a, b, IoU): identical boxes; equal axis-aligned boxes shifted by half their length, along x and along y: (L / 2) / (3 L / 2);
# the octagon over 2 - the octagon
CLOSED_FORMS = [
    ([3.0, 4.0, 4.0, 2.0, 0.7], [3.0, 4.0, 4.0, 2.0, 0.7], 1.0),
    ([0.0, 0.0, 4.0, 2.0, 0.0], [2.0, 0.0, 4.0, 2.0, 0.0], 1.0 / 3.0),
    ([1.0, -2.0, 4.0, 2.0, 0.0], [1.0, -1.0, 4.0, 2.0, 0.0], 1.0 / 3.0),
    ([0.0, 0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 1.0, 1.0, np.float32(np.pi / 4)], _OCT / (2.0 - _OCT)),
]


def _as7(box):
    """(cx, cy, dx, dy, heading) as the seven-column row corners_bev takes."""
    cx, cy, dx, dy, h = [float(v) for v in box]
    return (cx, cy, 0.0, dx, dy, 1.0, h)


def iou_pair_bev(a, b):
    """IoU of two rotated rectangles (cx, cy, dx, dy, heading), float64 from the float32 rows."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    if not (np.all(np.abs(a) < VALUE_LIMIT) and np.all(np.abs(b) < VALUE_LIMIT)):      # NaN and inf fail it too
        return 0.0
    if a[2] <= 0 or a[3] <= 0 or b[2] <= 0 or b[3] <= 0:
        return 0.0
    if math.hypot(a[0] - b[0], a[1] - b[1]) > 0.5 * (math.hypot(a[2], a[3]) + math.hypot(b[2], b[3])) + 1e-9:
        return 0.0
    inter = _area(_clip(corners_bev(_as7(a)), corners_bev(_as7(b))))
    union = a[2] * a[3] + b[2] * b[3] - inter
    if not inter > 0 or not union > 0:
        return 0.0
    return inter / union


def iou_matrix_bev(pd, gt):
    out = np.zeros((len(pd), len(gt)), dtype=np.float64)
    for i in range(len(pd)):
        for j in range(len(gt)):
            out[i, j] = iou_pair_bev(pd[i], gt[j])
    return out


def generate_waymo_type_results(infos, class_names, is_gt=False, fake_gt_infos=True):
    """waymo_eval2d.py:26-85 on a deep copy: columns [0, 1, 3, 4, 6] are taken after the fake-lidar conversion."""
    infos = copy.deepcopy(infos)
    frame_id, boxes2d, obj_type, score, overlap_nlz, difficulty = [], [], [], [], [], []
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
            b = info['gt_boxes_lidar']
            if fake_gt_infos:
                w, l, h, r = b[:, 3:4], b[:, 4:5], b[:, 5:6], b[:, 6:7]
                b[:, 2] += h[:, 0] / 2
                b = np.concatenate([b[:, 0:3], l, w, h, -(r + np.pi / 2)], axis=-1)
            boxes2d.append(b[box_mask][:, [0, 1, 3, 4, 6]])
        else:
            num_boxes = len(info['boxes_lidar'])
            difficulty.append([0] * num_boxes)
            score.append(info['score'])
            boxes2d.append(np.array(info['boxes_lidar'])[:, [0, 1, 3, 4, 6]])
            box_name = info['name']
        obj_type += [WAYMO_CLASSES.index(name) for name in box_name]
        frame_id.append(np.array([frame_index] * num_boxes))
        overlap_nlz.append(np.zeros(num_boxes))
    frame_id = np.concatenate(frame_id).reshape(-1).astype(np.int64)
    boxes2d = np.concatenate(boxes2d, axis=0)
    obj_type = np.array(obj_type).reshape(-1)
    score = np.concatenate(score).reshape(-1)
    overlap_nlz = np.concatenate(overlap_nlz).reshape(-1)
    difficulty = np.concatenate(difficulty).reshape(-1).astype(np.int8)
    boxes2d[:, -1] = limit_period(boxes2d[:, -1], offset=0.5, period=np.pi * 2)
    return frame_id, boxes2d, obj_type, score, overlap_nlz, difficulty


def evaluate_arrays(pd_frame, pd_boxes, pd_type, pd_score, gt_frame, gt_boxes, gt_type, gt_difficulty, n_frames,
                    thresholds=IOU_THRESHOLDS, pairs_fn=optimal_pairs):
    """counts [4][2][101][3] int64, ha [4][2][101] float64 and the per-problem IoU blocks of five-column boxes."""
    pd_boxes = np.asarray(pd_boxes, dtype=np.float32).reshape(-1, 5)
    gt_boxes = np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 5)
    pd_score = np.asarray(pd_score, dtype=np.float32)
    counts = np.zeros((4, 2, 101, 3), dtype=np.int64)
    ha = np.zeros((4, 2, 101), dtype=np.float64)
    blocks = []
    for f in range(n_frames):
        for t in (1, 2, 3, 4):
            pi = np.nonzero((pd_frame == f) & (pd_type == t))[0]
            gi = np.nonzero((gt_frame == f) & (gt_type == t))[0]
            order = pi[np.argsort(-pd_score[pi].astype(np.float64), kind='stable')]
            iou = iou_matrix_bev(pd_boxes[order], gt_boxes[gi])
            c, h = problem_counts(iou, pd_score[order], gt_difficulty[gi], pd_boxes[order, 4], gt_boxes[gi, 4],
                                  thresholds[t - 1], pairs_fn)
            counts[t - 1] += c
            ha[t - 1] += h
            blocks.append((f, t, order, gi, iou))
    return counts, ha, blocks


def waymo_evaluation(prediction_infos, gt_infos, class_name, distance_thresh=100, fake_gt_infos=True,
                     thresholds=IOU_THRESHOLDS):
    """waymo_eval2d.py:179-217 -> (result dict, counts, ha, IoU blocks)."""
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
    counts, ha, blocks = evaluate_arrays(pd_frame, pd_boxes, pd_type, pd_score, gt_frame, gt_boxes, gt_type, gt_diff,
                                         len(gt_infos), thresholds)
    return result_dict(counts, ha), counts, ha, blocks
