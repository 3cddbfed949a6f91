"""numpy restatement of Detector3DTemplate.generate_recall_record (cpd/models/detectors/detector3d_template.py:344-386) over the
oracle's boxes_iou3d, frame by frame, with no shortcuts: trimming loop, two IoU matrices, column maximum, strict `>`.
Independent of cpd_amd: the CPU tests pin it on the reference's own method (tests/golden/recall.npz), the GPU tests compare the
device kernel with it."""
import numpy as np


def record_keys(thresh_list):
    return ["gt"] + ["roi_%s" % str(t) for t in thresh_list] + ["rcnn_%s" % str(t) for t in thresh_list]


def trimmed_rows(gt):
    """l.358-362: rows 0 .. k count, k the last row whose float32 sum is not zero and never below 0; an empty block counts nothing."""
    gt = np.asarray(gt, np.float32)
    k = len(gt) - 1
    while k > 0 and gt[k].sum(dtype=np.float32) == 0:
        k -= 1
    return k + 1


def column_best(oracle, boxes, gt, n):
    """max IoU per counted gt over `boxes` (-1 when there is no box), -1 for rows not counted"""
    out = np.full(len(gt), -1.0, np.float32)
    boxes = np.asarray(boxes, np.float32)
    if n > 0 and boxes.size > 0:
        iou = oracle.boxes_iou3d(np.ascontiguousarray(boxes[:, :7]), np.ascontiguousarray(np.asarray(gt, np.float32)[:n, :7]))
        out[:n] = iou.max(axis=0)
    return out


def frame_record(oracle, pred, gt, rois, thresh_list):
    """-> (counters [1 + 2T] int64 in record_keys order, best_rcnn [M], best_roi [M], n_gt)"""
    gt = np.asarray(gt, np.float32)
    t = len(thresh_list)
    counters = np.zeros(1 + 2 * t, np.int64)
    n = trimmed_rows(gt)
    best_rcnn = column_best(oracle, pred, gt, n)
    best_roi = column_best(oracle, rois, gt, n) if rois is not None else np.full(len(gt), -1.0, np.float32)
    counters[0] = n
    for i, thr in enumerate(thresh_list):
        counters[1 + i] = int((best_roi[:n] > np.float32(thr)).sum())
        counters[1 + t + i] = int((best_rcnn[:n] > np.float32(thr)).sum())
    return counters, best_rcnn, best_roi, n


def batch_record(oracle, preds, gt_block, rois_block, thresh_list):
    """preds: list of [n_b, >= 7]; gt_block [B, M, ld]; rois_block [B, R, >= 7] or a list or None.
    -> (counters, best_rcnn [B, M], best_roi [B, M], n_gt [B])"""
    gt_block = np.asarray(gt_block, np.float32)
    b, m = gt_block.shape[:2]
    total = np.zeros(1 + 2 * len(thresh_list), np.int64)
    br, bo, ng = np.full((b, m), -1.0, np.float32), np.full((b, m), -1.0, np.float32), np.zeros(b, np.int32)
    for f in range(b):
        c, br[f], bo[f], ng[f] = frame_record(oracle, preds[f], gt_block[f], None if rois_block is None else rois_block[f], thresh_list)
        total += c
    return total, br, bo, ng


def split(concat, counts):
    """a concatenation [R, ld] + per-frame counts -> list of per-frame arrays"""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    return [concat[off[i]:off[i + 1]] for i in range(len(counts))]
