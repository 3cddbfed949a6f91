"""numpy restatement of the reference's test-time-augmentation fusion (TEST INFRASTRUCTURE; independent of cpd_amd):
DetectionsMerger.compute_WBF / merge_by_WBF (cpd/datasets/kitti/kitti_object_eval_python/merge_detections.py:110-228) and
model_nms_utils.compute_WBF (cpd/models/model_utils/model_nms_utils.py:5-113).

Inputs are float32 boxes [n, 7] and float32 scores [n], already floored and sorted; the caller's arrays are not modified. Every
number format is spelled out (float32 products and score sums, float64 accumulators), so the result does not depend on the scalar
promotion rules of the numpy at hand; where the reference leaves the format to numpy the rules of numpy >= 2 are meant.
`iou(a [1, 7], b [K, 7]) -> [1, K]` is the oracle's boxes_iou_bev (or the compiled reference's).

Every function returns (out_scores, out_boxes, cluster_of, trace):
  cluster_of [n] int32  the cluster a box joined (its creation index), DROPPED for a box the model variant discards, SINGLE for one it
                        emits on its own
  trace      list of (i, max_iou, runner_up_iou, n_clusters, decision) for every box but the first: what the margin checks read
"""
import numpy as np
import torch

f32 = np.float32
DROPPED, SINGLE = -1, -2
JOIN, OPEN, EMIT, DROP = "join", "open", "emit", "drop"
TWO_PI = 2 * np.pi


def limit_period(val, offset=0.5, period=np.pi):
    """common_utils.limit_period (cpd/utils/common_utils.py:17-20): torch float32 arithmetic"""
    val = torch.from_numpy(np.ascontiguousarray(val)).float()
    return (val - torch.floor(val / period + offset) * period).numpy()


def limit(ang):
    """model_nms_utils.limit (l.5-12) on a float32 array: numpy's float32 remainder, then the two folds"""
    ang = np.asarray(ang, f32) % f32(TWO_PI)
    ang[ang > f32(np.pi)] = ang[ang > f32(np.pi)] - f32(TWO_PI)
    ang[ang < f32(-np.pi)] = ang[ang < f32(-np.pi)] + f32(TWO_PI)
    return ang


def _step_ious(iou, box, merged):
    v = np.asarray(iou(box[None, :7], np.array(merged, f32).reshape(-1, 7)), f32)[0]
    k = int(np.argmax(v))                                        # the first maximum
    rest = np.delete(v, k)
    return k, f32(v[k]), f32(rest.max()) if rest.size else f32(-1.0)


def compute_wbf(scores, boxes, iou_thresh, iou, type="mean"):
    """merge_detections.py:110-181. The cluster's first list element and its merged box are one row of the reference's array, so a
    re-sum starts from the ALREADY MERGED box times the first score, not from the first member (l.151-157)."""
    boxes = np.array(boxes, f32).reshape(-1, 7)
    scores = np.array(scores, f32).reshape(-1)
    n = len(scores)
    cluster_of = np.zeros(n, np.int32)
    trace = []
    if n == 0:
        return scores, boxes, cluster_of, trace
    boxes[:, 6] = limit_period(boxes[:, 6], offset=0.5, period=TWO_PI)
    merged, members = [], []                                     # merged[k]: float32 [7]; members[k]: box indices
    thr = f32(iou_thresh)
    for i in range(n):
        if i > 0:
            k, v, second = _step_ious(iou, boxes[i], merged)
        if i > 0 and v > thr:
            trace.append((i, v, second, len(merged), JOIN))
            members[k].append(i)
            cluster_of[i] = k
            if type == "mean":
                acc = np.zeros(6, np.float64)
                ssum = f32(0)
                for pos, j in enumerate(members[k]):
                    row = merged[k][:6] if pos == 0 else boxes[j, :6]
                    acc += (row * scores[j]).astype(f32)          # float32 product, float64 sum, left to right
                    ssum = f32(ssum + scores[j])
                merged[k][:6] = (acc / np.float64(ssum)).astype(f32)
        else:
            if i > 0:
                trace.append((i, v, second, len(merged), OPEN))
            cluster_of[i] = len(merged)
            merged.append(boxes[i].copy())
            members.append([i])
    out_scores = []
    for m in members:
        if type == "mean":
            s = f32(0)
            for j in m:
                s = f32(s + scores[j])
            out_scores.append(f32(s / f32(len(m))))
        else:
            out_scores.append(np.max(scores[m]))
    return np.array(out_scores, f32), np.array(merged, f32).reshape(-1, 7), cluster_of, trace


def model_decision(v, score, thr, thr2, retain_low):
    """model_nms_utils.py:58-74, the five branches in order"""
    if v >= thr:
        return JOIN
    if thr2 <= v < thr and score > f32(0.4) and retain_low:
        return EMIT
    if f32(0.03) <= v < thr2 and retain_low:
        return DROP
    if (not retain_low) and f32(0.03) <= v < thr:
        return DROP
    return OPEN


def model_compute_wbf(scores, boxes, iou, iou_thresh=0.9, iou_thresh2=0.5, type="mean", retain_low=True):
    """model_nms_utils.py:14-113. -> out_scores / out_boxes in the reference's order (boxes emitted on their own first, in input order,
    then the clusters in creation order), cluster_of, trace, and the number of boxes emitted on their own as a fifth value."""
    boxes = np.array(boxes, f32).reshape(-1, 7)
    scores = np.array(scores, f32).reshape(-1)
    n = len(scores)
    cluster_of = np.zeros(n, np.int32)
    trace = []
    if n == 0:
        return scores, boxes, cluster_of, trace, 0
    boxes[:, 6] = limit(boxes[:, 6])
    thr, thr2 = f32(iou_thresh), f32(iou_thresh2)
    first, members = [], []
    out_scores, out_boxes = [], []
    for i in range(n):
        what = OPEN
        if i > 0:
            k, v, second = _step_ious(iou, boxes[i], [boxes[j] for j in first])
            what = model_decision(v, scores[i], thr, thr2, retain_low)
            trace.append((i, v, second, len(first), what))
        if what == JOIN:
            members[k].append(i)
            cluster_of[i] = k
        elif what == EMIT:
            out_scores.append(f32(f32(0.4) + f32(0.2) * f32(f32(scores[i] - f32(0.4)) / f32(0.6))))
            out_boxes.append(boxes[i].copy())
            cluster_of[i] = SINGLE
        elif what == DROP:
            cluster_of[i] = DROPPED
        else:
            cluster_of[i] = len(first)
            first.append(i)
            members.append([i])
    n_single = len(out_scores)
    for k, m in enumerate(members):
        box = boxes[first[k]].copy()
        if type == "mean":
            acc = np.zeros(6, np.float64)
            s = f32(0)
            for j in m:
                acc += boxes[j, :6]
                s = f32(s + scores[j])
            box[:6] = (acc / len(m)).astype(f32)
            res = limit(limit(boxes[m, 6]) - box[6])
            res = res[np.abs(res) < f32(1.5)]
            with np.errstate(invalid="ignore", divide="ignore"):
                box[6] = f32(box[6] + np_mean_f32(res))
            out_scores.append(f32(s / f32(len(m))))
        else:
            out_scores.append(np.max(scores[m]))
        out_boxes.append(box)
    return np.array(out_scores, f32), np.array(out_boxes, f32).reshape(-1, 7), cluster_of, trace, n_single


def np_mean_f32(a):
    """ndarray.mean of a float32 vector: numpy's pairwise float32 sum (eight running sums per block of up to 128 values, halves
    split at a multiple of eight beyond), divided by the count. Spelled out so the kernel's copy has a text to be read against;
    test_wbf_ref checks it against numpy itself."""
    a = np.asarray(a, f32)

    def pw(x):
        n = len(x)
        if n < 8:
            s = f32(0) if n == 0 else x[0]                        # (numpy starts a short sum at -0.0: the same values)
            for v in x[1:]:
                s = f32(s + v)
            return f32(s)
        if n <= 128:
            r = [x[j] for j in range(8)]
            i = 8
            while i < n - (n % 8):
                for j in range(8):
                    r[j] = f32(r[j] + x[i + j])
                i += 8
            s = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
            for v in x[i:]:
                s = f32(s + v)
            return s
        n2 = n // 2
        n2 -= n2 % 8
        return f32(pw(x[:n2]) + pw(x[n2:]))

    with np.errstate(invalid="ignore", divide="ignore"):
        return f32(pw(a) / f32(len(a)))


# ---- merge_by_WBF (merge_detections.py:184-228) -------------------------------------------------------------------------------------
def class_segment(names, scores, cls, floor):
    """l.195-207: indices of the boxes of class `cls` with score >= floor, by descending score (ties: ascending index)"""
    idx = np.flatnonzero((np.asarray(names) == cls) & (np.asarray(scores, f32) >= f32(floor)))
    return idx[np.argsort(-np.asarray(scores, f32)[idx], kind="stable")]


def merge_by_wbf(names, scores, boxes, cfg, iou, nms, classes=("Car", "Pedestrian", "Cyclist")):
    """cfg: dict with WBF_IOUS, WBF_PRE_SCORES, MERGE_TYPE, NMS_IOU. nms(boxes [m, 7], thresh) -> kept indices of the sorted boxes."""
    names, scores, boxes = np.asarray(names), np.asarray(scores, f32), np.asarray(boxes, f32).reshape(-1, 7)
    on, os_, ob = [], [], []
    for c, cls in enumerate(classes):
        idx = class_segment(names, scores, cls, cfg["WBF_PRE_SCORES"][c])
        kind = cfg["MERGE_TYPE"][c]
        if kind == "NMS":
            keep = np.asarray(nms(boxes[idx], cfg["NMS_IOU"]), np.int64) if len(idx) else np.zeros(0, np.int64)
            s, b = scores[idx][keep], boxes[idx][keep]
        else:
            s, b = compute_wbf(scores[idx], boxes[idx], cfg["WBF_IOUS"][c], iou, "mean" if kind == "WBF-mean" else "max")[:2]
        on.append(names[idx][:len(s)])
        os_.append(s)
        ob.append(b)
    return np.concatenate(on), np.concatenate(os_), np.concatenate(ob).reshape(-1, 7)


# ---- margins (what the exact comparisons rely on) -----------------------------------------------------------------------------------
def margins_ok(trace, thresholds, margin=1e-3):
    """every step's max IoU at least `margin` from every threshold, and a joining box's runner-up at least `margin` below"""
    for i, v, second, k, what in trace:
        for t in thresholds:
            if abs(float(v) - float(f32(t))) < margin:
                return False
        if what == JOIN and float(v) - float(second) < margin:
            return False
    return True


# ---- generated inputs ---------------------------------------------------------------------------------------------------------------
CLASS_SIZES = {"Car": (4.7, 2.1, 1.7), "Pedestrian": (0.9, 0.85, 1.75), "Cyclist": (1.8, 0.8, 1.7)}


def gen_detections(rng, n_obj, classes=("Car", "Pedestrian", "Cyclist"), jitter=1.0, views=(1, 6), n_isolated=3, n_low=3, heading=None,
                   spacing=10.0):
    """Base objects of the classes' sizes on a jittered grid, each seen in views[0] .. views[1] views with a small pose jitter, plus
    isolated boxes and boxes with scores below 0.05. Scores are distinct. -> names [n] str, scores [n] f32, boxes [n, 7] f32, in a
    random order (the order the views' result lists would be concatenated in does not matter to the fusion)."""
    side = int(np.ceil(np.sqrt(n_obj + n_isolated + n_low)))
    cells = rng.permutation(side * side)
    names, boxes = [], []

    def base(cell, cls):
        b = np.zeros(7)
        b[0] = (cell % side) * spacing - side * spacing / 2 + rng.uniform(-1, 1)
        b[1] = (cell // side) * spacing - side * spacing / 2 + rng.uniform(-1, 1)
        b[2] = rng.uniform(-1, 1)
        b[3:6] = np.array(CLASS_SIZES[cls]) * np.exp(rng.normal(0, 0.1, 3))
        b[6] = rng.uniform(-np.pi, np.pi) if heading is None else heading + rng.normal(0, 0.02)
        return b

    for o in range(n_obj):
        cls = classes[rng.integers(len(classes))]
        b = base(cells[o], cls)
        rel = rng.choice([0.02, 0.05, 0.1, 0.2]) * jitter                  # relative pose noise of this object's views
        for _ in range(rng.integers(views[0], views[1] + 1)):
            v = b.copy()
            v[:2] += rng.normal(0, 1, 2) * rel * b[3:5].min()
            v[2] += rng.normal(0, 0.05)
            v[3:6] *= np.exp(rng.normal(0, 0.3, 3) * rel)
            v[6] += rng.normal(0, 0.3) * rel + rng.choice([0, 0, 0, 2 * np.pi, -2 * np.pi])
            names.append(cls)
            boxes.append(v)
    for o in range(n_isolated + n_low):
        cls = classes[rng.integers(len(classes))]
        names.append(cls)
        boxes.append(base(cells[n_obj + o], cls))
    n = len(names)
    scores = (rng.permutation(n) + 1.0) / (n + 1.0) * 0.9 + 0.07              # distinct, in (0.07, 0.97)
    scores[n - n_low:] = 0.01 + 0.03 * (np.arange(n_low) + 1.0) / (n_low + 1.0)   # below every floor
    order = rng.permutation(n)
    return np.array(names)[order], scores.astype(f32)[order], np.array(boxes, f32).reshape(-1, 7)[order]


def sorted_segment(scores, boxes, floor=0.0):
    """the boxes with score >= floor by descending score: what compute_wbf takes"""
    idx = class_segment(np.zeros(len(scores), np.int8), scores, 0, floor)
    return np.asarray(scores, f32)[idx], np.asarray(boxes, f32).reshape(-1, 7)[idx]


def make_cluster(iou):
    """The restatement in the shape of cpd_amd.wbf.cluster_segments (boxes, scores, start, count, thresh, mode) ->
    (out_boxes [m, 7], out_scores [m], out_count [S], cluster_of [m]): what the tests inject in place of the launch."""
    def cluster(boxes, scores, start, count, thresh, mode):
        m = len(scores)
        ob, os_, cl = np.zeros((m, 7), f32), np.zeros(m, f32), np.full(m, -3, np.int32)
        oc = np.zeros(len(start), np.int32)
        for s, (a, c) in enumerate(zip(start, count)):
            kind = "max" if mode[s] & 1 else "mean"
            if mode[s] & 2:
                rs, rb, rc = model_compute_wbf(scores[a:a + c], boxes[a:a + c], iou, thresh[s][0], thresh[s][1], kind, not (mode[s] & 4))[:3]
            else:
                rs, rb, rc = compute_wbf(scores[a:a + c], boxes[a:a + c], thresh[s][0], iou, kind)[:3]
            oc[s] = len(rs)
            ob[a:a + len(rs)], os_[a:a + len(rs)], cl[a:a + c] = rb, rs, rc
        return ob, os_, oc, cl
    return cluster
