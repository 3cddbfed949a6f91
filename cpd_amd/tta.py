"""Test-time augmentation in one device step: every TEST_AUGMENTOR view of a batch of frames through an engine, and the views'
results fused, with no point and no box leaving the device in between.

The reference runs the detector once per view of the dataset config's TEST_AUGMENTOR (waymo_unsupervised_dbscan.yaml:84-139,
waymo_unsupervised_oyster.yaml:106-161: rotation 0 / +-0.3927, each with and without the x flip), maps every result list back
(TestAugmentor.backward) and fuses the lists with DetectionsMerger (merge_detections.py:76-228). `augmentor.TestAugmentor` and
`wbf.merge_frames` are those two ends with the host in between; this module is the same computation per chunk of frames as

    cpd_tta_views    the chunk's V views in one launch (csrc/tta.hip; TestAugmentor.forward's bits: the op arithmetic is shared)
    engine.forward   ONE step on the V * b view-major frames (its own count read-backs)
    cpd_tta_collect  backward transform + per-class floor + stable sort -> the segment table, on the device
    cpd_wbf_cluster  the WBF classes;  cpd_nms_batch  the NMS classes, on the same sorted segments
    one read-back of the per-segment COUNTS, then the classes of a frame concatenated in list order (device slices)

    tta = TTAEngine(engine, data_cfg["TEST_AUGMENTOR"], data_cfg["MERGE_CONFIG"], class_names)
    annos = tta.annos(tta.forward(points_list), frame_ids)           # -> waymo_eval / kitti_eval

Number formats are the host path's (csrc/tta_rules.h). One difference in the last place: where a view has a rotation other than 0,
the backward x / y are the unfused float32 products summed in a fixed order, while torch's host matmul associates and fuses as it
likes (a few units in the last place of max(|x|, |y|)); everything else, and every view without a rotation, is bit-equal."""
import collections
import ctypes

import numpy as np
import torch

from . import ops, wbf
from ._lib import check, lib, ptr, stream
from .augmentor import FLIP_X, FLIP_Y, MAX_OPS, ROT, SCALE, TestAugmentor, _get, rotation_cos_sin

MAX_VIEWS, MAX_CLASSES = 16, 16                                   # CPD_TTA_MAX_VIEWS, CPD_TTA_MAX_CLASSES
_KIND_MODE = {"WBF-mean": wbf.MODE_MEAN, "WBF-max": wbf.MODE_MAX, "NMS": wbf.MODE_NMS}

Segments = collections.namedtuple("Segments", "boxes scores src start count count_wbf count_nms thresh mode")


def _queue(aug, back):
    """(name, config) of a TestAugmentor's forward or reversed queue"""
    return [(p.func.__name__, p.keywords["config"]) for p in (aug.test_back_queue if back else aug.data_augmentor_queue)]


def view_ops(aug):
    """The point ops of TestAugmentor.forward, as cpd_augment_scene takes them: [(kind, p0, p1), ...]"""
    out = []
    for name, cfg in _queue(aug, False):
        if name == "world_flip":
            axis = _get(cfg, "ALONG_AXIS")
            if axis in ("x", "y"):
                out.append((FLIP_X if axis == "x" else FLIP_Y, 0.0, 0.0))
        elif name == "world_rotation":
            out.append((ROT,) + rotation_cos_sin(_get(cfg, "WORLD_ROT")))
        else:
            out.append((SCALE, float(_get(cfg, "WORLD_SCALE")), 0.0))
    return out


def back_ops(aug):
    """The box ops of TestAugmentor.backward (the reversed queue): [(kind, p0, p1, p2), ...]; a rotation carries the float32 cos / sin
    the host derives for -WORLD_ROT and the angle itself."""
    out = []
    for name, cfg in _queue(aug, True):
        if name == "world_flip":
            axis = _get(cfg, "ALONG_AXIS")
            if axis in ("x", "y"):
                out.append((FLIP_X if axis == "x" else FLIP_Y, 0.0, 0.0, 0.0))
        elif name == "world_rotation":
            rot = _get(cfg, "WORLD_ROT")
            out.append((ROT,) + rotation_cos_sin(-rot) + (float(-rot),))
        else:
            out.append((SCALE, float(_get(cfg, "WORLD_SCALE")), 0.0, 0.0))
    return out


def _op_tables(op_lists, width):
    """kind [V][MAX_OPS] i32, param [V][MAX_OPS][width] f64, n [V] i32 (a list longer than MAX_OPS keeps its length: the library
    reports it)"""
    v = len(op_lists)
    kind, param = np.zeros((max(v, 1), MAX_OPS), np.int32), np.zeros((max(v, 1), MAX_OPS, width), np.float64)
    n = np.array([len(o) for o in op_lists] or [0], np.int32)
    for i, lst in enumerate(op_lists):
        for q, op in enumerate(lst[:MAX_OPS]):
            kind[i, q] = op[0]
            param[i, q] = op[1:]
    return kind, param, n


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def views(points_list, test_augmentors):
    """cpd_tta_views: the frames `points_list` ([n_f, c] float32 device tensors of one width) through every TestAugmentor of
    `test_augmentors` in one launch, queued on the current stream. -> the V * B view-major list (v0f0, v0f1, .., v1f0, ..) an engine
    takes; entry v * B + f is bit-equal to test_augmentors[v].forward({"points": points_list[f]})["points"] and a slice of one
    allocation. Nothing is filtered, reordered or read back."""
    batch, n_views = len(points_list), len(test_augmentors)
    packed = points_list[0].contiguous() if batch == 1 else torch.cat(list(points_list), 0)
    assert packed.dtype == torch.float32 and packed.dim() == 2 and packed.is_cuda
    n_total, c = int(packed.shape[0]), int(packed.shape[1])
    offsets = np.zeros(batch + 1, np.int64)
    offsets[1:] = np.cumsum([int(p.shape[0]) for p in points_list])
    kind, param, n_ops = _op_tables([view_ops(a) for a in test_augmentors], 2)
    fits = 0 < n_views <= MAX_VIEWS and n_views * n_total < 2 ** 31
    out = torch.empty((n_views * n_total if fits else 0, c), dtype=torch.float32, device=packed.device)     # (the library reports the limit)
    check(lib().cpd_tta_views(ptr(packed), n_total, c, _vp(offsets), batch, _vp(kind), _vp(param), _vp(n_ops), n_views, ptr(out), stream()),
          "cpd_tta_views")
    return [out[v * n_total + offsets[f]:v * n_total + offsets[f + 1]] for v in range(n_views) for f in range(batch)]


def _class_tables(merge_cfg, class_names):
    floors = np.ascontiguousarray([wbf._cfg(merge_cfg, "WBF_PRE_SCORES")[c] for c in range(len(class_names))], np.float32)
    ious = np.ascontiguousarray([wbf._cfg(merge_cfg, "WBF_IOUS")[c] for c in range(len(class_names))], np.float32)
    modes = np.ascontiguousarray([_KIND_MODE[wbf._cfg(merge_cfg, "MERGE_TYPE")[c]] for c in range(len(class_names))], np.int32)
    return floors, ious, modes


def _collect(entry, tail, boxes, scores, labels, counts, test_augmentors, merge_cfg, class_names, batch):
    n_views, n_class = len(test_augmentors), len(class_names)
    boxes, scores, labels, counts = boxes.contiguous(), scores.contiguous(), labels.contiguous(), counts.contiguous()
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and labels.dtype == torch.int64 and counts.dtype == torch.int32
    assert boxes.dim() == 3 and boxes.shape[2] == 7 and boxes.shape[0] == n_views * batch == counts.numel()
    cap = int(boxes.shape[1])
    assert scores.numel() == n_views * batch * cap == labels.numel()
    kind, param, n_back = _op_tables([back_ops(a) for a in test_augmentors], 3)
    floors, ious, modes = _class_tables(merge_cfg, class_names)
    s, vk = batch * n_class, n_views * cap
    fits = 0 < n_views <= MAX_VIEWS and n_class <= MAX_CLASSES and s * vk < 2 ** 31
    rows = vk if fits else 0                                      # (the library reports the limit)
    dev = boxes.device

    def words(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev)
    seg = Segments(torch.zeros((s, rows, 7), dtype=torch.float32, device=dev), torch.zeros((s, rows), dtype=torch.float32, device=dev),
                   torch.full((s, rows), -1, dtype=torch.int32, device=dev), words(s), words(s), words(s), words(s),
                   torch.zeros((s, 2), dtype=torch.float32, device=dev), words(s))
    check(entry(ptr(boxes), ptr(scores), ptr(labels), ptr(counts), n_views, batch, cap, _vp(kind), _vp(param), _vp(n_back), _vp(floors),
                _vp(ious), _vp(modes), n_class, ptr(seg.boxes), ptr(seg.scores), ptr(seg.src), ptr(seg.start), ptr(seg.count),
                ptr(seg.count_wbf), ptr(seg.count_nms), ptr(seg.thresh), ptr(seg.mode), *tail), entry.__name__)
    return seg


def collect(boxes, scores, labels, counts, test_augmentors, merge_cfg, class_names, batch):
    """cpd_tta_collect, queued on the current stream, nothing read back. The engine's results for the view-major batch of `views` as
    padded device blocks: boxes [V * batch, K, 7] float32, scores [V * batch, K] float32, labels [V * batch, K] int64 (1-based), counts
    [V * batch] int32. -> Segments, segment s = frame * len(class_names) + class: boxes [S, V K, 7] mapped back by the view's
    TestAugmentor.backward, scores [S, V K] and src [S, V K] (the candidate slot view * K + row) floored at WBF_PRE_SCORES and by
    descending score (ties: the lower slot), start / count / thresh / mode as cpd_wbf_cluster reads them for boxes.view(-1, 7),
    count_wbf / count_nms = count for the classes MERGE_TYPE sends to WBF / NMS and 0 for the others. count -1: more than
    wbf.MAX_SEGMENT boxes passed the floor."""
    ops._need_cuda(boxes, "boxes")
    return _collect(lib().cpd_tta_collect, (stream(),), boxes, scores, labels, counts, test_augmentors, merge_cfg, class_names, batch)


def collect_cpu(boxes, scores, labels, counts, test_augmentors, merge_cfg, class_names, batch):
    """cpd_tta_collect_cpu: collect's rules on the calling thread, HOST tensors in and out (no device needed)."""
    assert not boxes.is_cuda
    return _collect(lib().cpd_tta_collect_cpu, (), boxes, scores, labels, counts, test_augmentors, merge_cfg, class_names, batch)


def check_segments(counts):
    """ValueError, as wbf raises it, when a segment was refused (host list of Segments.count)"""
    if min(counts, default=0) < 0:
        raise ValueError("cpd_tta_collect refused a segment (longer than %d boxes; raise the score floor)" % wbf.MAX_SEGMENT)


def fuse(seg, merge_cfg, class_names, batch):
    """The fusion of collect's segments on the device: cpd_wbf_cluster on the WBF classes, cpd_nms_batch on the NMS classes, ONE
    read-back of the per-segment counts, then per frame the classes in list order (device slices / gathers). -> per frame
    {"pred_boxes" [k, 7], "pred_scores" [k], "pred_labels" [k] int64} on the device."""
    n_class = len(class_names)
    s, vk = seg.scores.shape
    dev = seg.boxes.device
    modes = _class_tables(merge_cfg, class_names)[2]
    ob, os_, oc, _ = ops.wbf_cluster(seg.boxes.view(-1, 7), seg.scores.view(-1), seg.start, seg.count_wbf, seg.thresh, seg.mode)
    ob, os_ = ob.view(s, vk, 7), os_.view(s, vk)
    parts = [seg.count, oc]
    if (modes == wbf.MODE_NMS).any():
        keep, n_keep = ops.nms_batch(seg.boxes, seg.count_nms, float(wbf._cfg(merge_cfg, "NMS_IOU")))
        parts.append(n_keep)
    host = torch.cat(parts).tolist()                              # the step's one read-back here: counts only
    check_segments(host[:s])
    out = []
    for f in range(batch):
        fb, fs, fl = [], [], []
        for c in range(n_class):
            i = f * n_class + c
            if modes[c] == wbf.MODE_NMS:
                idx = keep[i, :host[2 * s + i]]
                fb.append(seg.boxes[i].index_select(0, idx))
                fs.append(seg.scores[i].index_select(0, idx))
            else:
                k = host[s + i]
                fb.append(ob[i, :k])
                fs.append(os_[i, :k])
            fl.append(torch.full((fs[-1].shape[0],), c + 1, dtype=torch.int64, device=dev))
        out.append({"pred_boxes": torch.cat(fb) if fb else torch.zeros((0, 7), device=dev),
                    "pred_scores": torch.cat(fs) if fs else torch.zeros((0,), device=dev),
                    "pred_labels": torch.cat(fl) if fl else torch.zeros((0,), dtype=torch.int64, device=dev)})
    return out


class TTAEngine:
    """points [N, C] per frame -> the fused detections of all TEST_AUGMENTOR views per frame.

    engine: a CenterPointEngine, or a VoxelRCNNEngine with either first stage, built with host_results=False. test_augmentor_cfg: the
    yaml's TEST_AUGMENTOR list (one AUG_CONFIG_LIST per view). merge_cfg: WBF_IOUS, WBF_PRE_SCORES, MERGE_TYPE, NMS_IOU, as for
    wbf.merge_frames. Frames are taken in chunks of max_batch // V, so that an engine step sees at most max_batch frames."""

    def __init__(self, engine, test_augmentor_cfg, merge_cfg, class_names, max_batch=48, host_results=False):
        if getattr(engine, "host_results", False):
            raise ValueError("TTAEngine: the engine must keep its results on the device (host_results=False)")
        self.engine = engine
        self.class_names = list(class_names)
        self.merge_cfg = merge_cfg
        self.host_results = bool(host_results)
        self.augmentors = [TestAugmentor(_get(view, "AUG_CONFIG_LIST", view), self.class_names) for view in test_augmentor_cfg]
        n_views = len(self.augmentors)
        if not 0 < n_views <= MAX_VIEWS or len(self.class_names) > MAX_CLASSES:
            raise ValueError("TTAEngine: 1 .. %d views and at most %d classes" % (MAX_VIEWS, MAX_CLASSES))
        if max_batch < n_views:
            raise ValueError("TTAEngine: max_batch %d is less than the %d views of one frame" % (max_batch, n_views))
        self.chunk = int(max_batch) // n_views

    @torch.no_grad()
    def forward(self, points_list):
        if isinstance(points_list, torch.Tensor):
            points_list = [points_list]
        out = []
        for at in range(0, len(points_list), self.chunk):
            frames = points_list[at:at + self.chunk]
            self.engine.forward(views(frames, self.augmentors))
            seg = collect(*self.engine.last_result_block, self.augmentors, self.merge_cfg, self.class_names, len(frames))
            out += fuse(seg, self.merge_cfg, self.class_names, len(frames))
        if self.host_results and out:                             # one copy: boxes, scores and labels of all frames as one block
            ns = [int(r["pred_scores"].shape[0]) for r in out]
            blk = torch.cat([torch.cat([r["pred_boxes"], r["pred_scores"][:, None], r["pred_labels"][:, None].float()], 1) for r in out]).cpu()
            cut = np.cumsum([0] + ns)
            out = [{"pred_boxes": blk[a:b, :7], "pred_scores": blk[a:b, 7], "pred_labels": blk[a:b, 8].long()} for a, b in zip(cut[:-1], cut[1:])]
        return out

    __call__ = forward

    def annos(self, results, frame_ids):
        """forward's results -> the per-frame `name` / `score` / `boxes_lidar` (+ `frame_id`) list waymo_eval and kitti_eval take"""
        names = np.array(self.class_names)
        out = []
        for r, fid in zip(results, frame_ids):
            labels = r["pred_labels"].cpu().numpy()
            out.append({"name": names[labels - 1] if len(labels) else names[:0], "score": r["pred_scores"].cpu().numpy(),
                        "boxes_lidar": r["pred_boxes"].cpu().numpy().reshape(-1, 7), "frame_id": fid})
        return out
