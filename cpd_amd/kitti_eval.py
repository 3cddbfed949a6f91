"""KITTI-protocol 3D detection evaluation on the GPU: a drop-in for
cpd/datasets/kitti/kitti_object_eval_python/eval.py (and its rotate_iou.py), with no JIT compiler dependency.

Same public surface and the same return values: get_official_eval_result(gt_annos, dt_annos, current_classes,
PR_detail_dict=None) -> (result string, ret_dict), and the helpers it is built from. Inputs are kitti_common
annotation dicts of numpy arrays, as Kitti2WaymoDataset builds them (cpd_amd.kitti2waymo.generate_prediction_dicts makes the detections' side).

Where the work runs:
  * overlaps (image IoU, BEV rotated IoU, 3-D IoU) of every frame: one cpd_kitti_overlaps launch per metric;
  * compute_statistics_jit's matching: one cpd_kitti_match_scores launch (the scores get_thresholds reads) and one
    cpd_kitti_match_pr launch (tp / fp / fn / similarity per threshold, summed over frames) per metric, covering every
    (class, difficulty, min_overlap) sweep of that metric -- a full get_official_eval_result is nine launches plus copies;
  * clean_data / _prepare_data (class and difficulty flags, DontCare boxes) stay on the host, vectorised; get_thresholds
    and the recall / precision / AOS arithmetic stay float64 on the host, in the reference's order.

Differences from the reference, all deliberate:
  * its debug prints (eval.py:26 in get_thresholds, eval.py:621-622 in do_eval) are not reproduced;
  * overlaps are computed per frame (the reference also computes, then discards, cross-frame blocks); calculate_iou_partly
    still returns the reference's per-part matrices;
  * annotation arrays are read as float64 (BEV boxes as float32, as the reference casts them), and the image, DontCare
    and 3-D overlaps are computed in float64. The reference's jitted code instead specialises on the arrays' dtypes. For
    all-float64 annotations (kitti_common.get_label_annos; every test here) each value is the reference's. The caller
    this module replaces, Kitti2WaymoDataset.evaluation, passes mixed dtypes: kitti_infos gts hold float32 `bbox` and
    `location` (object3d_kitti's box2d / loc) beside float64 `dimensions`, `rotation_y` and `alpha`; predictions hold
    float32 `bbox`, `location`, `dimensions` and `score`, while a frame with no detection holds float64 zeros. There the
    reference computes some image overlaps, the DontCare overlaps and the 3-D volumes in float32, or in float64 rounded
    to float32, per part of frames. Its overlaps can then differ from these by about one float32 step (~6e-8 near
    0.5), so a detection whose overlap lies that close to 0.25 / 0.5 / 0.7 can match differently. Every other value
    (BEV overlaps, matching given the overlaps, thresholds, AP arithmetic) is the reference's;
  * the jitted np.sum adds the AOS terms sequentially; so does the kernel (numpy's pairwise sum would differ in the last bit).
Where the reference raises, this raises: a (class, difficulty) with no valid gt divides by zero in get_thresholds
(ZeroDivisionError), and more than 41 thresholds overflow the precision arrays (IndexError).
"""
import numpy as np
import torch

from . import _lib

N_SAMPLE_PTS = 41
CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'truck']
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]


# ---- device plumbing ------------------------------------------------------------------------------------------------

def _device():
    if not torch.cuda.is_available():
        raise _lib.CpdHipError("cpd_amd.kitti_eval needs a GPU: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_device())


def _offsets(counts, dtype=np.int32):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=off[1:])
    return off.astype(dtype)


def _segmented_overlaps(metric, criterion, rows, cols, row_counts, col_counts):
    """Packed row x col blocks of consecutive segments (device float64) and their offsets (host int64)."""
    row_counts = np.asarray(row_counts, dtype=np.int64)
    col_counts = np.asarray(col_counts, dtype=np.int64)
    pair_off = _offsets(row_counts * col_counts, np.int64)
    n_pairs = int(pair_off[-1])
    if row_counts.sum() > np.iinfo(np.int32).max or col_counts.sum() > np.iinfo(np.int32).max:
        raise _lib.CpdHipError("kitti_eval: more than 2^31 boxes")
    dtype = np.float32 if metric == 1 else np.float64
    d_rows, d_cols = _to_dev(rows, dtype), _to_dev(cols, dtype)
    d_roff, d_coff = _to_dev(_offsets(row_counts), np.int32), _to_dev(_offsets(col_counts), np.int32)
    d_poff = _to_dev(pair_off, np.int64)
    out = torch.empty(max(n_pairs, 1), dtype=torch.float64, device=_device())
    lib = _lib.lib()
    _lib.check(lib.cpd_kitti_overlaps(metric, criterion, _lib.ptr(d_rows), _lib.ptr(d_cols), _lib.ptr(d_roff),
                                      _lib.ptr(d_coff), _lib.ptr(d_poff), len(row_counts), n_pairs, _lib.ptr(out),
                                      _lib.stream()), "cpd_kitti_overlaps")
    return out, pair_off


def _blocks(packed, pair_off, row_counts, col_counts):
    host = packed.cpu().numpy()
    return [host[pair_off[f]:pair_off[f + 1]].reshape(int(row_counts[f]), int(col_counts[f]))
            for f in range(len(row_counts))]


# ---- overlaps (eval.py:91-155, rotate_iou.py:295-330) ---------------------------------------------------------------

def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """iou[n, k] = devRotateIoUEval(query_boxes[k], boxes[n], criterion) of float32 (x, y, dx, dy, angle) boxes;
    criterion -1 IoU, 0 over the query box's area, 1 over the box's area, 2 raw intersection area. float32 [N, K]."""
    boxes = np.asarray(boxes).astype(np.float32)
    query_boxes = np.asarray(query_boxes).astype(np.float32)
    N, K = boxes.shape[0], query_boxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=np.float32)
    with torch.cuda.device(device_id):
        out, _ = _segmented_overlaps(1, int(criterion), boxes, query_boxes, [N], [K])
        return out.cpu().numpy().reshape(N, K).astype(np.float32)


def image_box_overlap(boxes, query_boxes, criterion=-1):
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    N, K = boxes.shape[0], query_boxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=boxes.dtype)
    out, _ = _segmented_overlaps(0, int(criterion), boxes, query_boxes, [N], [K])
    return out.cpu().numpy().reshape(N, K).astype(boxes.dtype)


def bev_box_overlap(boxes, qboxes, criterion=-1):
    return rotate_iou_gpu_eval(boxes, qboxes, criterion)


def d3_box_overlap(boxes, qboxes, criterion=-1):
    """Camera boxes (x, y, z, l, h, w, ry): the float32 BEV intersection of columns (0, 2, 3, 5, 6) times the height
    overlap, over the union (criterion -1) -- float32 [N, K] like the reference's rinc."""
    boxes, qboxes = np.asarray(boxes), np.asarray(qboxes)
    N, K = boxes.shape[0], qboxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=np.float32)
    out, _ = _segmented_overlaps(2, int(criterion), boxes, qboxes, [N], [K])
    return out.cpu().numpy().reshape(N, K).astype(np.float32)


def _metric_boxes(annos, metric):
    if metric == 0:
        return np.concatenate([a["bbox"] for a in annos], 0).astype(np.float64).reshape(-1, 4)
    if metric == 1:
        loc = np.concatenate([a["location"][:, [0, 2]] for a in annos], 0)
        dims = np.concatenate([a["dimensions"][:, [0, 2]] for a in annos], 0)
        rots = np.concatenate([a["rotation_y"] for a in annos], 0)
        return np.concatenate([loc, dims, rots[..., np.newaxis]], axis=1).astype(np.float32)
    if metric == 2:
        loc = np.concatenate([a["location"] for a in annos], 0)
        dims = np.concatenate([a["dimensions"] for a in annos], 0)
        rots = np.concatenate([a["rotation_y"] for a in annos], 0)
        return np.concatenate([loc, dims, rots[..., np.newaxis]], axis=1).astype(np.float64)
    raise ValueError("unknown metric")


def _part_sizes(n, num_parts):
    """Frames per part of calculate_iou_partly: num_parts equal parts of n // num_parts frames, plus one part with the
    remainder if any; a single part when n < num_parts."""
    size, rest = divmod(n, num_parts)
    if size == 0:
        return [n]
    return [size] * num_parts + ([rest] if rest else [])


def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50):
    """The reference's (overlaps, parted_overlaps, total_gt_num, total_dt_num): per-part [sum gt, sum dt] matrices
    (rows = the FIRST argument's boxes) and every frame's block of them. float64, except metric 0 which keeps the
    first argument's bbox dtype as image_box_overlap does."""
    assert len(gt_annos) == len(dt_annos)
    gt_num = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
    dt_num = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
    frame_off = _offsets(_part_sizes(len(gt_annos), num_parts), np.int64)
    part_gt = np.add.reduceat(gt_num, frame_off[:-1]) if len(gt_num) else np.zeros(1, np.int64)
    part_dt = np.add.reduceat(dt_num, frame_off[:-1]) if len(dt_num) else np.zeros(1, np.int64)
    rows, cols = _metric_boxes(gt_annos, metric), _metric_boxes(dt_annos, metric)
    packed, pair_off = _segmented_overlaps(metric, -1, rows, cols, part_gt, part_dt)
    parted = _blocks(packed, pair_off, part_gt, part_dt)
    if metric == 0:
        dtype = np.concatenate([a["bbox"] for a in gt_annos], 0).dtype
        parted = [p.astype(dtype) for p in parted]
    # frame f of part p: rows / columns from its offset within the part
    overlaps = []
    for p, block in enumerate(parted):
        frames = slice(frame_off[p], frame_off[p + 1])
        r_off, c_off = _offsets(gt_num[frames], np.int64), _offsets(dt_num[frames], np.int64)
        overlaps += [block[r_off[k]:r_off[k + 1], c_off[k]:c_off[k + 1]] for k in range(len(r_off) - 1)]
    return overlaps, parted, gt_num, dt_num


# ---- host half of the protocol --------------------------------------------------------------------------------------

def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """Score thresholds of the recall sample points (eval.py:8-27, without its print). Walking the scores from high to
    low, a score is kept when the recall it reaches is at least as close to the next sample point as the recall one score
    later (the last score is always kept); each kept score moves the sample point up by 1 / (num_sample_pts - 1).
    Between two kept scores the sample point is fixed, so the next one is found by one vectorised search: at most about
    num_sample_pts searches, with the same float64 expressions in the same order as a score-by-score walk."""
    if num_gt == 0:
        raise ZeroDivisionError("division by zero")     # the reference divides by num_gt (l.26) even with no scores
    ordered = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    count = len(ordered)
    rank = np.arange(1, count + 1, dtype=np.int64)
    recall_here = rank / num_gt
    recall_next = (rank + 1) / num_gt
    if count:
        recall_next[-1] = recall_here[-1]
    can_skip = rank < count
    step = 1 / (num_sample_pts - 1.0)
    sample, kept, pos = 0, [], 0
    while pos < count:
        later = (recall_next[pos:] - sample) < (sample - recall_here[pos:])
        pos += int(np.argmin(later & can_skip[pos:]))    # first score that is kept
        kept.append(ordered[pos])
        sample += step
        pos += 1
    return kept


def _names(annos):
    parts = [np.asarray(a["name"]).astype(str) for a in annos if len(a["name"])]
    return np.concatenate(parts) if parts else np.zeros(0, dtype="<U1")


def _cat(annos, key, shape_tail=()):
    parts = [np.asarray(a[key], dtype=np.float64).reshape((-1,) + shape_tail) for a in annos]
    return np.concatenate(parts, 0) if parts else np.zeros((0,) + shape_tail)


class _Frames:
    """clean_data / _prepare_data (eval.py:30-88, 418-448) for every (class, difficulty) at once, as flat arrays."""

    def __init__(self, gt_annos, dt_annos, current_classes, difficultys):
        assert len(gt_annos) == len(dt_annos)
        self.n_frames = len(gt_annos)
        self.gt_num = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
        self.dt_num = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
        gt_names, dt_names = _names(gt_annos), _names(dt_annos)
        gt_lower, dt_lower = np.char.lower(gt_names), np.char.lower(dt_names)
        gt_bbox, dt_bbox = _cat(gt_annos, "bbox", (4,)), _cat(dt_annos, "bbox", (4,))
        occluded, truncated = _cat(gt_annos, "occluded"), _cat(gt_annos, "truncated")
        gt_height = gt_bbox[:, 3] - gt_bbox[:, 1]
        dt_height = np.abs(dt_bbox[:, 3] - dt_bbox[:, 1])
        self.ig_gt = np.empty((len(current_classes) * len(difficultys), len(gt_names)), dtype=np.int8)
        self.ig_dt = np.empty((len(current_classes) * len(difficultys), len(dt_names)), dtype=np.int8)
        self.num_valid_gt = np.zeros(self.ig_gt.shape[0], dtype=np.int64)
        for m, class_id in enumerate(current_classes):
            cls = CLASS_NAMES[class_id].lower()
            valid_gt = np.where(gt_lower == cls, 1, -1)
            if cls == "pedestrian":
                valid_gt[gt_lower == "person_sitting"] = 0
            elif cls == "car":
                valid_gt[gt_lower == "van"] = 0
            valid_dt = dt_lower == cls
            for l, level in enumerate(difficultys):
                ignore = ((occluded > MAX_OCCLUSION[level]) | (truncated > MAX_TRUNCATION[level])
                          | (gt_height <= MIN_HEIGHT[level]))
                ig = np.full(len(gt_names), -1, dtype=np.int8)
                ig[(valid_gt == 0) | (ignore & (valid_gt == 1))] = 1
                ig[(valid_gt == 1) & ~ignore] = 0
                cd = m * len(difficultys) + l
                self.ig_gt[cd] = ig
                self.num_valid_gt[cd] = int(np.count_nonzero(ig == 0))
                igd = np.where(valid_dt, 0, -1).astype(np.int8)
                igd[dt_height < MIN_HEIGHT[level]] = 1
                self.ig_dt[cd] = igd
        dc = gt_names == "DontCare"
        frame_of_gt = np.repeat(np.arange(self.n_frames), self.gt_num)
        self.dc_num = np.bincount(frame_of_gt[dc], minlength=self.n_frames).astype(np.int64)
        self.dc_bbox = gt_bbox[dc]
        self.dt_bbox = dt_bbox
        self.dt_score = _cat(dt_annos, "score")
        self.dt_alpha = _cat(dt_annos, "alpha")
        self.gt_alpha = _cat(gt_annos, "alpha")


def _sweep_list(n_class, difficultys, min_overlaps, metric):
    """(class slot m, difficulty slot l, overlap slot k, flag row m * n_difficulty + l, min_overlap) in eval_class order."""
    n_diff, n_ov = len(difficultys), min_overlaps.shape[0]
    return [(m, l, k, m * n_diff + l, float(min_overlaps[k, metric, m]))
            for m in range(n_class) for l in range(n_diff) for k in range(n_ov)]


class _MetricRun:
    """Device state of one metric: per-frame overlaps and the sweep tables both matching passes read."""

    def __init__(self, frames, gt_annos, dt_annos, metric, sweeps):
        self.fr, self.metric, self.sweeps = frames, metric, sweeps
        self.overlaps, pair_off = _segmented_overlaps(metric, -1, _metric_boxes(dt_annos, metric),
                                                      _metric_boxes(gt_annos, metric), frames.dt_num, frames.gt_num)
        self.pair_off = pair_off
        self.d_pair_off = _to_dev(pair_off, np.int64)
        self.d_dt_off = _to_dev(_offsets(frames.dt_num), np.int32)
        self.d_gt_off = _to_dev(_offsets(frames.gt_num), np.int32)
        self.d_dc_off = _to_dev(_offsets(frames.dc_num), np.int32)
        self.d_ig_gt, self.d_ig_dt = _to_dev(frames.ig_gt, np.int8), _to_dev(frames.ig_dt, np.int8)
        self.d_score = _to_dev(frames.dt_score, np.float64)
        self.d_sweep_cd = _to_dev([s[3] for s in sweeps], np.int32)
        self.d_sweep_ov = _to_dev([s[4] for s in sweeps], np.float64)
        self.total_gt, self.total_dt = int(frames.gt_num.sum()), int(frames.dt_num.sum())
        ws = _lib.lib().cpd_kitti_match_workspace_bytes(len(sweeps), frames.n_frames, self.total_dt)
        self.workspace = torch.empty(max(ws, 1), dtype=torch.uint8, device=_device())
        self.ws_bytes = ws

    def matched_scores(self):
        """Pass 1: (scores, matched) [n_sweeps, total_gt] on the host."""
        S = len(self.sweeps)
        scores = torch.empty((S, max(self.total_gt, 1)), dtype=torch.float64, device=_device())
        matched = torch.empty((S, max(self.total_gt, 1)), dtype=torch.int8, device=_device())
        P = _lib.ptr
        _lib.check(_lib.lib().cpd_kitti_match_scores(
            P(self.overlaps), P(self.d_pair_off), P(self.d_dt_off), P(self.d_gt_off), self.fr.n_frames, P(self.d_ig_gt),
            P(self.d_ig_dt), P(self.d_score), P(self.d_sweep_cd), P(self.d_sweep_ov), S, self.total_gt, self.total_dt,
            P(scores), P(matched), P(self.workspace), self.ws_bytes, _lib.stream()), "cpd_kitti_match_scores")
        return scores[:, :self.total_gt].cpu().numpy(), matched[:, :self.total_gt].cpu().numpy().astype(bool)

    def pr(self, thresholds, compute_aos):
        """Pass 2: pr [n_sweeps, 41, 4] float64 (tp, fp, fn, similarity) for the sweeps' threshold lists."""
        S = len(self.sweeps)
        thr = np.zeros((S, N_SAMPLE_PTS), dtype=np.float64)
        n_thr = np.zeros(S, dtype=np.int32)
        for s, t in enumerate(thresholds):
            thr[s, :len(t)] = t
            n_thr[s] = len(t)
        counts = torch.empty((S, N_SAMPLE_PTS, 3), dtype=torch.int64, device=_device())
        sim = torch.empty((S, N_SAMPLE_PTS), dtype=torch.float64, device=_device())
        fr, P = self.fr, _lib.ptr
        d_dt_alpha, d_gt_alpha = _to_dev(fr.dt_alpha, np.float64), _to_dev(fr.gt_alpha, np.float64)
        d_dt_bbox, d_dc_bbox = _to_dev(fr.dt_bbox, np.float64), _to_dev(fr.dc_bbox, np.float64)
        d_thr, d_nthr = _to_dev(thr, np.float64), _to_dev(n_thr, np.int32)
        _lib.check(_lib.lib().cpd_kitti_match_pr(
            P(self.overlaps), P(self.d_pair_off), P(self.d_dt_off), P(self.d_gt_off), P(self.d_dc_off), fr.n_frames,
            P(self.d_ig_gt), P(self.d_ig_dt), P(self.d_score), P(d_dt_alpha), P(d_gt_alpha), P(d_dt_bbox), P(d_dc_bbox),
            self.metric, int(bool(compute_aos)), P(self.d_sweep_cd), P(self.d_sweep_ov), P(d_thr), P(d_nthr), S,
            self.total_gt, self.total_dt, P(counts), P(sim), P(self.workspace), self.ws_bytes, _lib.stream()),
            "cpd_kitti_match_pr")
        pr = np.zeros((S, N_SAMPLE_PTS, 4), dtype=np.float64)
        pr[:, :, :3] = counts.cpu().numpy()
        pr[:, :, 3] = sim.cpu().numpy()
        return pr


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False,
               num_parts=100):
    """eval.py:451-560: dict of recall, precision and aos [num_class, num_difficulty, num_minoverlap, 41].
    num_parts only shaped the reference's host batching; the result does not depend on it."""
    assert len(gt_annos) == len(dt_annos)
    frames = _Frames(gt_annos, dt_annos, current_classes, difficultys)
    sweeps = _sweep_list(len(current_classes), difficultys, min_overlaps, metric)
    run = _MetricRun(frames, gt_annos, dt_annos, metric, sweeps)
    scores, matched = run.matched_scores()
    thresholds = []
    for s, (m, l, k, cd, _) in enumerate(sweeps):
        t = np.array(get_thresholds(scores[s][matched[s]], int(frames.num_valid_gt[cd])))
        if len(t) > N_SAMPLE_PTS:
            raise IndexError("index %d is out of bounds for axis 3 with size %d" % (N_SAMPLE_PTS, N_SAMPLE_PTS))
        thresholds.append(t)
    pr = run.pr(thresholds, compute_aos)
    shape = [len(current_classes), len(difficultys), len(min_overlaps), N_SAMPLE_PTS]
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s, (m, l, k, cd, _) in enumerate(sweeps):
            T = len(thresholds[s])
            p = pr[s, :T]
            recall[m, l, k, :T] = p[:, 0] / (p[:, 0] + p[:, 2])
            precision[m, l, k, :T] = p[:, 0] / (p[:, 0] + p[:, 1])
            if compute_aos:
                aos[m, l, k, :T] = p[:, 3] / (p[:, 0] + p[:, 1])
            # precision[i] = max(precision[i:]) for i < T, in place from i = 0: a suffix maximum of the values above
            precision[m, l, k, :T] = np.maximum.accumulate(precision[m, l, k, ::-1])[::-1][:T]
            if compute_aos:
                aos[m, l, k, :T] = np.maximum.accumulate(aos[m, l, k, ::-1])[::-1][:T]
    return {"recall": recall, "precision": precision, "orientation": aos}


def _sampled_ap(prec, samples):
    """Mean of prec[..., samples] in percent. The samples are added one at a time, left to right, then divided by
    their count and scaled: the order the protocol's AP values are defined in, so they come out bit for bit."""
    acc = np.zeros(prec.shape[:-1])
    for i in samples:
        acc = acc + prec[..., i]
    return acc / len(samples) * 100


def get_mAP(prec):
    """11-point AP: recall samples 0, 4, ..., 40 of the 41."""
    return _sampled_ap(prec, range(0, prec.shape[-1], 4))


def get_mAP_R40(prec):
    """40-point AP: every recall sample but the first."""
    return _sampled_ap(prec, range(1, prec.shape[-1]))


# (PR_detail_dict / result key, eval_class metric) in the order the protocol evaluates them
_METRICS = (("bbox", 0), ("bev", 1), ("3d", 2))


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, PR_detail_dict=None):
    """(bbox, bev, 3d, aos, bbox_R40, bev_R40, 3d_R40, aos_R40) AP arrays [num_class, 3, num_minoverlap]; the aos
    pair is None unless compute_aos (orientation similarity is taken on the image-box metric only)."""
    ap, ap40 = {}, {}
    for key, metric in _METRICS:
        with_aos = compute_aos and metric == 0
        res = eval_class(gt_annos, dt_annos, current_classes, [0, 1, 2], metric, min_overlaps, with_aos)
        curves = [(key, res["precision"])] + ([("aos", res["orientation"])] if with_aos else [])
        for name, curve in curves:
            ap[name], ap40[name] = get_mAP(curve), get_mAP_R40(curve)
            if PR_detail_dict is not None:
                PR_detail_dict[name] = curve
    return tuple(table.get(k) for table in (ap, ap40) for k in ("bbox", "bev", "3d", "aos"))


# min_overlaps [2 sets, 3 metrics (bbox, bev, 3d), 6 classes]: the protocol's thresholds
_MIN_OVERLAPS = np.array([[[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3,
                          [[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5],
                           [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]]])
_CLASS_LABELS = ("Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Truck")
_DIFFICULTY_NAMES = ("easy", "moderate", "hard")
# result-string rows: (AP table key, line label, decimals)
_RESULT_ROWS = (("bbox", "bbox AP", 4), ("bev", "bev  AP", 4), ("3d", "3d   AP", 4), ("aos", "aos  AP", 2))
# ret_dict entries per class, all from the 40-point AP at the first overlap set: (AP table key, key stem)
_RET_ROWS = (("aos", "aos"), ("3d", "3d"), ("bev", "bev"), ("bbox", "image"))


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None):
    """(result string, ret_dict) of the KITTI protocol for the given classes (names or indices)."""
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    class_ids = {label: i for i, label in enumerate(_CLASS_LABELS)}
    classes = [class_ids[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = _MIN_OVERLAPS[:, :, classes]
    # orientation is scored when the first detection list that has entries carries a real alpha (not the -10 filler)
    first_alpha = next((a["alpha"] for a in dt_annos if a["alpha"].shape[0] != 0), None)
    compute_aos = first_alpha is not None and first_alpha[0] != -10
    aps = do_eval(gt_annos, dt_annos, classes, min_overlaps, compute_aos, PR_detail_dict=PR_detail_dict)
    ap = dict(zip(("bbox", "bev", "3d", "aos"), aps[:4]))
    ap40 = dict(zip(("bbox", "bev", "3d", "aos"), aps[4:]))

    lines, ret_dict = [], {}
    for j, cls in enumerate(classes):
        label = _CLASS_LABELS[cls]
        for i in range(min_overlaps.shape[0]):
            thresholds = ", ".join(format(v, ".2f") for v in min_overlaps[i, :, j])
            for heading, table in (("AP", ap), ("AP_R40", ap40)):
                lines.append("%s %s@%s:" % (label, heading, thresholds))
                for key, row_label, digits in _RESULT_ROWS:
                    if table[key] is not None:
                        lines.append(row_label + ":" + ", ".join(format(table[key][j, d, i], ".%df" % digits)
                                                                 for d in range(3)))
        for key, stem in _RET_ROWS:
            if ap40[key] is not None:
                for d, diff in enumerate(_DIFFICULTY_NAMES):
                    ret_dict["%s_%s/%s_R40" % (label, stem, diff)] = ap40[key][j, d, 0]
    return "".join(line + "\n" for line in lines), ret_dict
