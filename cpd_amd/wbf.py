"""Fusion of test-time-augmentation views: the step between `TestAugmentor.backward` and `waymo_eval` / `kitti_eval`.

The reference merges the result lists of its TEST_AUGMENTOR views with DetectionsMerger
(cpd/datasets/kitti/kitti_object_eval_python/merge_detections.py:76-228; compute_WBF of merge_detections_tracking.py:121-191 is the
same text): per class a score floor, a sort by score, then weighted box fusion (`WBF-mean` / `WBF-max`) or `nms_gpu`. The model
package carries a second variant (cpd/models/model_utils/model_nms_utils.py:14-113) for the consumer of post_processing's
`WBF: True` branch. Both are Python loops that rebuild the cluster list and call a 1 x K CPU IoU for every box. Here every
(frame, class) is one segment of ONE cpd_wbf_cluster launch (csrc/wbf.hip): one workgroup per segment, lanes over the clusters.

    views = [engine_results_of_view(v) for v in test_augmentor.views]      # each mapped back by TestAugmentor.backward,
    infos = merge_frames(views, cfg.MERGE_CONFIG, class_names)             # each a generate_prediction_dicts list
    OpenPCDetWaymoDetectionMetricsEstimator().waymo_evaluation(infos, gt_infos, class_names)

Number formats are the reference's under numpy >= 2 (a float32 scalar stays float32 against a Python number): float32 boxes and
scores, float32 products, float64 sums; see csrc/wbf_rules.h. Deviation from the reference, on purpose: the caller's arrays are
NOT modified (the reference writes the folded headings and the merged boxes into its argument).
"""
import collections
import copy

import numpy as np
import torch

from . import ops

MODE_MEAN, MODE_MAX, MODE_MODEL, MODE_NO_RETAIN = 0, 1, 2, 4      # CPD_WBF_* of include/cpd_hip.h
MODE_NMS = -1                                                     # segment table only: the class goes through nms_gpu
MAX_SEGMENT = 8192                                                # CPD_WBF_MAX_SEGMENT
LDS_CLUSTERS = 512                                                # CPD_WBF_LDS_CLUSTERS
BLOCK = 256                                                       # CPD_WBF_BLOCK
DROPPED, SINGLE = -1, -2                                          # cluster_of codes of the model variant

SegmentTable = collections.namedtuple("SegmentTable", "order start count thresh mode frame cls")


def _host(x, dtype=None):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a if dtype is None else np.ascontiguousarray(a, dtype)


def _boxes7(x):
    """columns 0:7 of a box table as contiguous float32 (an empty table may come without its second dimension)"""
    a = _host(x, np.float32)
    if a.ndim != 2:
        a = a.reshape(-1, 7)
    return np.ascontiguousarray(a[:, :7])


def _cfg(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def _check_count(n, what):
    if n > MAX_SEGMENT:
        raise ValueError("%s: a segment of %d boxes; cpd_wbf_cluster takes at most %d per frame and class (raise the score floor)"
                         % (what, n, MAX_SEGMENT))


def segment_order(names, scores, cls, floor):
    """merge_detections.py:195-207: the boxes of class `cls` with score >= floor (float32 comparison), by descending score; ties by
    ascending index (the reference's np.argsort(-scores) leaves them open)."""
    idx = np.flatnonzero((names == cls) & (scores >= np.float32(floor)))
    return idx[np.argsort(-scores[idx], kind="stable")]


def build_segment_table(frames, merge_cfg, classes):
    """Pure host: the segments of all frames. `frames`: list of (names, scores) per frame, the views already concatenated in view
    order. One segment per (frame, class) in that order, empty ones included: rows `order[start : start + count]` of the
    concatenation of all frames; thresh [S, 2] = (WBF_IOUS[c], 0); mode = MODE_MEAN / MODE_MAX / MODE_NMS by MERGE_TYPE[c]."""
    ious, floors, kinds = _cfg(merge_cfg, "WBF_IOUS"), _cfg(merge_cfg, "WBF_PRE_SCORES"), _cfg(merge_cfg, "MERGE_TYPE")
    kind_mode = {"WBF-mean": MODE_MEAN, "WBF-max": MODE_MAX, "NMS": MODE_NMS}
    order, start, count, thresh, mode, frame, cls_of = [], [], [], [], [], [], []
    base = at = 0
    for f, (names, scores) in enumerate(frames):
        names, scores = _host(names), _host(scores, np.float32)
        for c, cls in enumerate(classes):
            idx = segment_order(names, scores, cls, floors[c])
            m = kind_mode[kinds[c]]
            if m != MODE_NMS:
                _check_count(len(idx), "frame %d, class %s" % (f, cls))
            order.append(idx + base)
            start.append(at)
            count.append(len(idx))
            thresh.append((ious[c], 0.0))
            mode.append(m)
            frame.append(f)
            cls_of.append(c)
            at += len(idx)
        base += len(names)
    return SegmentTable(np.concatenate(order).astype(np.int64) if order else np.zeros(0, np.int64), np.array(start, np.int32),
                        np.array(count, np.int32), np.array(thresh, np.float32).reshape(-1, 2), np.array(mode, np.int32),
                        np.array(frame, np.int32), np.array(cls_of, np.int32))


def cluster_segments(boxes, scores, start, count, thresh, mode, device="cuda"):
    """One upload, one cpd_wbf_cluster launch, one read-back. boxes [m, 7] / scores [m] float32 host arrays, every segment floored
    and sorted; start / count / mode int32 [S], thresh float32 [S, 2].
    -> (out_boxes [m, 7], out_scores [m], out_count [S], cluster_of [m]) host arrays, each segment's results from its start row."""
    m, s = len(scores), len(start)
    parts = [np.ascontiguousarray(boxes, np.float32).reshape(-1).view(np.int32), np.ascontiguousarray(scores, np.float32).view(np.int32),
             np.ascontiguousarray(thresh, np.float32).reshape(-1).view(np.int32), np.ascontiguousarray(start, np.int32),
             np.ascontiguousarray(count, np.int32), np.ascontiguousarray(mode, np.int32)]
    assert parts[0].size == 7 * m and parts[2].size == 2 * s and parts[4].size == s and parts[5].size == s
    dev = torch.device(device)
    buf = torch.from_numpy(np.concatenate(parts)).to(dev)
    cut = np.cumsum([0] + [p.size for p in parts])
    d = [buf[cut[i]:cut[i + 1]] for i in range(6)]
    out = torch.zeros((9 * m + s,), dtype=torch.int32, device=dev)
    ob, os_, cl, oc = out[:7 * m], out[7 * m:8 * m], out[8 * m:9 * m], out[9 * m:]
    cl.fill_(-3)
    ops.wbf_cluster(d[0].view(torch.float32), d[1].view(torch.float32), d[3], d[4], d[2].view(torch.float32), d[5],
                    out_boxes=ob.view(torch.float32), out_scores=os_.view(torch.float32), out_count=oc, cluster_of=cl)
    host = out.cpu().numpy()
    got = (host[:7 * m].view(np.float32).reshape(m, 7), host[7 * m:8 * m].view(np.float32), host[9 * m:], host[8 * m:9 * m])
    if (got[2] < 0).any():
        raise ValueError("cpd_wbf_cluster refused a segment (out of range or longer than %d boxes)" % MAX_SEGMENT)
    return got


def cluster_segments_host(boxes, scores, start, count, thresh, mode):
    """cluster_segments without a device: the same rules on the calling thread (cpd_wbf_cluster_cpu), same arguments and results.
    Pass it as `_cluster=` to the functions below to fuse on a host that has no GPU."""
    t = [torch.from_numpy(np.ascontiguousarray(a, d)) for a, d in ((boxes, np.float32), (scores, np.float32), (start, np.int32),
                                                                   (count, np.int32), (thresh, np.float32), (mode, np.int32))]
    got = tuple(x.numpy() for x in ops.wbf_cluster_cpu(*t))
    if (got[2] < 0).any():
        raise ValueError("cpd_wbf_cluster_cpu refused a segment (out of range or longer than %d boxes)" % MAX_SEGMENT)
    return got


def _nms_device(boxes, scores, thresh):
    """merge_detections.py:93-108: nms_gpu on the class's sorted boxes -> kept positions, best first"""
    from . import iou3d_nms_utils
    dev = torch.device("cuda")
    keep = iou3d_nms_utils.nms_gpu(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), thresh)[0]
    return keep.cpu().numpy()


def _one_segment(det_names, det_scores, det_boxes, thresh, mode, cluster, what):
    boxes = _boxes7(det_boxes)
    scores = _host(det_scores, np.float32).reshape(-1)
    n = len(scores)
    _check_count(n, what)
    ob, os_, oc, cl = (cluster or cluster_segments)(boxes, scores, np.zeros(1, np.int32), np.array([n], np.int32),
                                                    np.array([thresh], np.float32), np.array([mode], np.int32))
    return ob[:oc[0]].copy(), os_[:oc[0]].copy(), cl


def _like(ref, arr):
    return torch.from_numpy(arr).to(ref.device) if isinstance(ref, torch.Tensor) else arr


def compute_WBF(det_names, det_scores, det_boxes, iou_thresh, type='mean', _cluster=None):
    """DetectionsMerger.compute_WBF (merge_detections.py:110-181), same return triple (names, scores, boxes): the boxes, taken in
    the order given (merge_by_WBF sorts them), join the cluster of largest BEV IoU when that is > iou_thresh, else open one; 'mean'
    moves the cluster box to the score-weighted mean (with the reference's aliasing: the running mean stands in for the first member)
    and returns mean scores, 'max' keeps the first box and the largest score. numpy arrays or tensors; float32; the inputs are not
    modified. ValueError above MAX_SEGMENT boxes."""
    if len(det_names) == 0:
        return det_names, det_scores, det_boxes
    mode = {"mean": MODE_MEAN, "max": MODE_MAX}[type]
    boxes, scores, _ = _one_segment(det_names, det_scores, det_boxes, (iou_thresh, 0.0), mode, _cluster, "compute_WBF")
    return det_names[0:len(scores)], _like(det_scores, scores), _like(det_boxes, boxes)


def model_compute_WBF(det_names, det_scores, det_boxes, iou_thresh=0.9, iou_thresh2=0.5, type='mean', retain_low=True, _cluster=None):
    """model_nms_utils.compute_WBF (model_nms_utils.py:14-113), same return triple: clusters stay at their first member while
    clustering; a box joins at IoU >= iou_thresh, is emitted on its own with a damped score between the thresholds (score > 0.4,
    retain_low), is dropped at 0.03 <= IoU below that, and opens a cluster otherwise; 'mean' returns the members' unweighted mean
    with the first heading moved by the mean residual. Output: the boxes emitted on their own, then the clusters."""
    if len(det_names) == 0:
        return det_names, det_scores, det_boxes
    mode = MODE_MODEL | {"mean": MODE_MEAN, "max": MODE_MAX}[type] | (0 if retain_low else MODE_NO_RETAIN)
    boxes, scores, cl = _one_segment(det_names, det_scores, det_boxes, (iou_thresh, iou_thresh2), mode, _cluster, "model_compute_WBF")
    names = _host(det_names)
    n_clusters = int(cl.max(initial=-1)) + 1
    first = np.full(n_clusters, len(cl), np.int64)
    np.minimum.at(first, cl[cl >= 0], np.flatnonzero(cl >= 0))
    out_names = np.concatenate([names[cl == SINGLE], names[first]])
    return out_names, _like(det_scores, scores), _like(det_boxes, boxes)


def _merge(frames, merge_cfg, classes, cluster, nms):
    """frames: list of (names, scores, boxes) -> list of (names, scores, boxes) merged per frame, classes concatenated in order"""
    if not frames:
        return []
    frames = [(_host(n), _host(s, np.float32).reshape(-1), _boxes7(b)) for n, s, b in frames]
    table = build_segment_table([(n, s) for n, s, _ in frames], merge_cfg, classes)
    names = np.concatenate([f[0] for f in frames]) if frames else np.zeros(0, "<U1")
    scores = np.concatenate([f[1] for f in frames])[table.order]
    boxes = np.ascontiguousarray(np.concatenate([f[2] for f in frames]).reshape(-1, 7)[table.order])
    names = names[table.order]
    wbf = np.flatnonzero(table.mode != MODE_NMS)
    ob, os_, oc, _ = (cluster or cluster_segments)(boxes, scores, table.start[wbf], table.count[wbf], table.thresh[wbf], table.mode[wbf])
    n_out = np.zeros(len(table.start), np.int64)
    n_out[wbf] = oc
    out = []
    for f in range(len(frames)):
        fn, fs, fb = [], [], []
        for s in np.flatnonzero(table.frame == f):
            a, c = int(table.start[s]), int(table.count[s])
            if table.mode[s] == MODE_NMS:
                if c == 0:
                    continue
                keep = np.asarray((nms or _nms_device)(boxes[a:a + c], scores[a:a + c], _cfg(merge_cfg, "NMS_IOU")), np.int64)
                fn.append(names[a:a + c][keep]); fs.append(scores[a:a + c][keep]); fb.append(boxes[a:a + c][keep])
            else:
                k = int(n_out[s])
                fn.append(names[a:a + k]); fs.append(os_[a:a + k]); fb.append(ob[a:a + k])
        out.append((np.concatenate(fn) if fn else names[:0], np.concatenate(fs) if fs else scores[:0],
                    np.concatenate(fb).reshape(-1, 7) if fb else boxes[:0]))
    return out


def merge_by_WBF(det_names, det_scores, det_boxes, merge_cfg, classes=('Car', 'Pedestrian', 'Cyclist'), _cluster=None, _nms=None):
    """DetectionsMerger.merge_by_WBF (merge_detections.py:184-228) for one frame: per class of `classes` the score floor
    WBF_PRE_SCORES[c] (>=), the sort, then MERGE_TYPE[c]: 'WBF-mean' / 'WBF-max' at WBF_IOUS[c], or 'NMS' at NMS_IOU through
    iou3d_nms_utils.nms_gpu. The classes' results are concatenated in list order. `merge_cfg`: a dict or an attribute object.
    -> (names, scores float32, boxes float32 [k, 7]) numpy."""
    return _merge([(det_names, det_scores, det_boxes)], merge_cfg, classes, _cluster, _nms)[0]


def merge_frames(view_infos, merge_cfg, classes=('Car', 'Pedestrian', 'Cyclist'), _cluster=None, _nms=None):
    """DetectionsMerger.prepare_detections + merge (merge_detections.py:76-91,231-241) for a whole split. `view_infos`: a list over
    the views of the per-frame annotation lists of generate_prediction_dicts (`name`, `score`, `boxes_lidar`; already mapped back
    by TestAugmentor.backward). Per frame the views are concatenated in view order; the segment table of all frames and WBF classes
    is built on the host (build_segment_table), then one upload, one clustering launch, one read-back. Returns a deep copy of view
    0's list with `name`, `score`, `boxes_lidar` replaced, ready for waymo_eval / kitti_eval.
    Out of scope: the KITTI camera fields of merge() (l.243-255: calibration files, image boxes, alpha / bbox / dimensions / location /
    rotation_y, and its in-place z += h / 2 on the stored boxes_lidar); those keys keep view 0's values."""
    n_frames = len(view_infos[0])
    assert all(len(v) == n_frames for v in view_infos), "merge_frames: every view lists the same frames"
    frames = []
    for f in range(n_frames):
        frames.append((np.concatenate([_host(v[f]["name"]) for v in view_infos]),
                       np.concatenate([_host(v[f]["score"], np.float32).reshape(-1) for v in view_infos]),
                       np.concatenate([_boxes7(v[f]["boxes_lidar"]) for v in view_infos])))
    merged = _merge(frames, merge_cfg, classes, _cluster, _nms)
    out = copy.deepcopy(view_infos[0])
    for f, (names, scores, boxes) in enumerate(merged):
        out[f]["name"], out[f]["score"], out[f]["boxes_lidar"] = names, scores, boxes
    return out
