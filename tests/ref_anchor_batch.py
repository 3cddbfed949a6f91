"""Host statement of cpd_anchor_assign_batch (AxisAlignedTargetAssigner.assign_targets for a whole batch) on the CPU oracle, and the
inputs the CPU and GPU tests of it share. Per frame: trim the trailing all-zero rows (at least one row stays), give every row to the
anchor set of class_names[int(c) - 1] -- Python's index wrap included, so class id 0 lands in the LAST class --, run
oracle.anchor_assign per (frame, set) and put the results into the reference's layout: each set viewed as (outer, inner[, 7]) with
outer = anchors.shape[0] * anchors.shape[1], the sets concatenated along `inner`."""
import numpy as np

CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
SMALL_RANGE = [0.0, -10.0, -2.0, 20.0, 10.0, 4.0]
SMALL_GRID = [11, 9]                                                # x = 0, 2, ..., 20; y = -10, -7.5, ..., 10


def small_cfgs():
    """The three classes of voxel_rcnn_dbscan_single_train.yaml."""
    return [dict(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0], align_center=False,
                 feature_map_stride=8, matched_threshold=mt, unmatched_threshold=ut)
            for n, s, mt, ut in (("Vehicle", [4.7, 2.1, 1.7], 0.55, 0.5), ("Pedestrian", [0.91, 0.86, 1.73], 0.55, 0.4),
                                 ("Cyclist", [1.78, 0.84, 1.78], 0.55, 0.4))]


def V(x, y, ry, s=1.0):
    return [x, y, 0, 4.7 * s, 2.1 * s, 1.7, ry, 1]


def P(x, y, ry):
    return [x, y, 0, .9, .85, 1.7, ry, 2]


def C(x, y, ry):
    return [x, y, 0, 1.8, .8, 1.7, ry, 3]


def small_gt():
    """[5][8][8], zero padded: a full frame, a duplicated box, an empty frame, an all-zero row between boxes, a box off the grid."""
    frames = [[P(8, 2.5, .3), V(4.3, .2, .1), C(10.3, -2.4, .05), V(13, -1.25, 0), P(15.1, 6, 1.2), V(8.9, 5.4, 1.5, .9), C(17, -7.5, 1.6)],
              [P(6, -5, 0), P(6, -5, 0)],
              [],
              [V(10, 0, 0), [0] * 8, C(4, 5, 0)],
              [V(100, 100, 0), P(2.2, 7.4, 0)]]
    gt = np.zeros((len(frames), 8, 8), np.float32)
    for b, rows in enumerate(frames):
        for j, row in enumerate(rows):
            gt[b, j] = row
    return gt


def thresholds(cfgs):
    return {c["class_name"]: (c["matched_threshold"], c["unmatched_threshold"]) for c in cfgs}


def frame_rows(gt_frame, class_names, anchor_class_names):
    """Row numbers of one frame's gt [M][ld] per anchor set, after the trim (axis_aligned_target_assigner.py:66-69, 83-84)."""
    nz = np.nonzero(np.abs(gt_frame[:, :-1]).sum(1))[0]
    cnt = int(nz[-1]) + 1 if len(nz) else 1
    cls = gt_frame[:cnt, -1].astype(np.int32)
    return [np.array([j for j in range(min(cnt, len(gt_frame))) if class_names[int(cls[j]) - 1] == name], np.int64)
            for name in anchor_class_names]


def ref_anchor_batch(oracle, anchor_sets, gt, class_names, anchor_class_names, thr, norm_by_num_examples=False):
    """anchor_sets: per class a numpy array shaped like the reference's anchors (feature_map_size = shape[:2], last axis 7);
    gt [B][M][ld]; thr = {class name: (matched, unmatched)}. Returns labels / gt_ious / reg_weights [B][N], reg_targets [B][N][7],
    gt_max_iou [B][M], n_examples [B][sets] and rows[b][s] = the row numbers set s received in frame b."""
    B, M = gt.shape[:2]
    outer = [a.shape[0] * a.shape[1] for a in anchor_sets]
    assert len(set(outer)) == 1
    flat = [np.ascontiguousarray(a.reshape(-1, 7), np.float32) for a in anchor_sets]
    out = {k: [] for k in ("labels", "reg_targets", "reg_weights", "gt_ious")}
    gt_max = np.zeros((B, M), np.float32)
    n_examples = np.zeros((B, len(flat)), np.int32)
    rows = []
    for b in range(B):
        rows.append(frame_rows(gt[b], class_names, anchor_class_names))
        per_set = []
        for s, (name, a) in enumerate(zip(anchor_class_names, flat)):
            sel = gt[b][rows[b][s]]
            lab, tgt, w, iou = oracle.anchor_assign(a, sel[:, :7], sel[:, -1].astype(np.int32), thr[name][0], thr[name][1],
                                                    norm_by_num_examples)
            if len(sel):
                gt_max[b, rows[b][s]] = oracle.nearest_bev_iou(a, sel[:, :7]).max(0)
            n_examples[b, s] = int((lab >= 0).sum())
            per_set.append((lab, tgt, w, iou))
        o = outer[0]
        out["labels"].append(np.concatenate([t[0].reshape(o, -1) for t in per_set], -1).reshape(-1))
        out["reg_targets"].append(np.concatenate([t[1].reshape(o, -1, 7) for t in per_set], -2).reshape(-1, 7))
        out["reg_weights"].append(np.concatenate([t[2].reshape(o, -1) for t in per_set], -1).reshape(-1))
        out["gt_ious"].append(np.concatenate([t[3].reshape(o, -1) for t in per_set], -1).reshape(-1))
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(gt_max_iou=gt_max, n_examples=n_examples, rows=rows)
    return res


def set_columns(anchor_sets, s):
    """Columns of set s in a frame's row of the assembled layout, in the set's own anchor order."""
    inner = [a.reshape(-1, 7).shape[0] // (a.shape[0] * a.shape[1]) for a in anchor_sets]
    outer = anchor_sets[0].shape[0] * anchor_sets[0].shape[1]
    r, q = np.divmod(np.arange(outer * inner[s]), inner[s])
    return r * sum(inner) + sum(inner[:s]) + q
