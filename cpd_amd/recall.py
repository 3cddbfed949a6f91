"""The eval-time recall record on the device: Detector3DTemplate.generate_recall_record
(cpd/models/detectors/detector3d_template.py:344-386), which both post_processing bodies call once per frame
(detector3d_template.py:326-330, cpd/models/detectors/centerpoint.py:36-50) and whose counters
tools/eval_utils/eval_utils.py:14-21,94-101 sums, shows on the progress bar and logs as recall_roi_<t> / recall_rcnn_<t>.

The reference builds two N x M IoU matrices per frame and waits for the device once per threshold, per side and per trailing
padded gt row. Here a batch is ONE cpd_recall_record launch (csrc/iou3d_nms.hip) that adds into a device counter tensor; nothing
waits until somebody reads the numbers (`RecallRecord.as_dict`).

    rec = RecallRecord(cfg.MODEL.POST_PROCESSING.RECALL_THRESH_LIST)
    for batch in loader:
        ...
        rec.update(final_boxes, None, final_counts, batch['gt_boxes'], rois=batch['rois'])    # queued, no wait
    rec.reduce_()                      # distributed evaluation: the sum merge_results_dist + eval_utils.py:88-92 take
    rec.as_dict()                      # {'gt': .., 'roi_0.3': .., 'rcnn_0.3': .., ...}: the reference's recall_dict
    rec.summary()                      # {'recall/roi_0.3': .., 'recall/rcnn_0.3': .., ...}: eval_utils.py:94-101
"""
import numpy as np
import torch

from . import ops

DEFAULT_THRESH_LIST = (0.3, 0.5, 0.7)       # RECALL_THRESH_LIST of every shipped model yaml


def record_keys(thresh_list):
    """The reference's keys in the order of the device counters: gt, roi_<t> .., rcnn_<t> .. (`str(t)` as at l.355-356)."""
    return ["gt"] + ["roi_%s" % str(t) for t in thresh_list] + ["rcnn_%s" % str(t) for t in thresh_list]


def pad_gt(boxes_per_frame, ld=None):
    """The collated gt block of a batch (cpd/datasets/dataset.py collate_batch: zero rows behind each frame's boxes):
    list of [n_b, ld] arrays / tensors -> float32 tensor [B, max n_b, ld] on the host."""
    arrays = [np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b, np.float32) for b in boxes_per_frame]
    arrays = [a.reshape(0, ld or 8) if a.size == 0 and a.ndim < 2 else a for a in arrays]
    if ld is None:
        ld = max([a.shape[1] for a in arrays if a.shape[0]] + [arrays[0].shape[1] if arrays else 8])
    out = np.zeros((len(arrays), max([a.shape[0] for a in arrays] + [0]), ld), np.float32)
    for b, a in enumerate(arrays):
        assert a.shape[0] == 0 or a.shape[1] == ld, "pad_gt: frames disagree on the row length"
        out[b, :a.shape[0]] = a
    return torch.from_numpy(out)


class RecallRecord:
    """The recall counters of one evaluation on the device (int64 [1 + 2 * len(thresh_list)]: gt, roi_<t> .., rcnn_<t> ..).
    They accumulate over `update` calls as the reference's dict does over the frames of a batch and the batches of an epoch."""

    def __init__(self, thresh_list=DEFAULT_THRESH_LIST, device="cuda"):
        self.thresh_list = list(thresh_list)
        if not 1 <= len(self.thresh_list) <= 8:
            raise ValueError("RecallRecord: 1..8 thresholds, got %d" % len(self.thresh_list))
        self.thresh = [float(t) for t in self.thresh_list]
        self.keys = record_keys(self.thresh_list)
        self.device = torch.device(device)
        self.counters = torch.zeros((len(self.keys),), dtype=torch.int64, device=self.device)
        self._blocks = {}                  # (batch, capacity) -> (start, full count) of a padded block
        self._dummy = None

    # ---- addressing ------------------------------------------------------------------------------------------------
    def _block(self, batch, cap):
        hit = self._blocks.get((batch, cap))
        if hit is None:
            start = torch.arange(batch, dtype=torch.int32, device=self.device) * cap
            hit = self._blocks[(batch, cap)] = (start, torch.full((batch,), cap, dtype=torch.int32, device=self.device))
        return hit

    def _rows(self, boxes, start, count, batch, what):
        """-> (float32 rows on the device, start [B] int32, count [B] int32) of a padded [B, cap, ld] block (start / count optional),
        of a concatenation [R, ld] with its start / count, or of a list of per-frame tensors."""
        if isinstance(boxes, (list, tuple)):
            assert len(boxes) == batch, "%s: one tensor per frame" % what
            ns = [int(b.shape[0]) for b in boxes]
            kept = [b[:, :7] for b in boxes if b.shape[0]]
            boxes = torch.cat(kept, dim=0) if kept else None
            host = np.array([np.cumsum([0] + ns[:-1]), ns], np.int32)
            dev = torch.from_numpy(host).to(self.device)
            start, count = dev[0], dev[1]
        elif boxes.dim() == 3:
            assert boxes.shape[0] == batch, "%s: a padded block has one slab per frame" % what
            blk_start, blk_count = self._block(batch, boxes.shape[1])
            start = blk_start if start is None else start
            count = blk_count if count is None else count
        else:
            assert boxes.dim() == 2 and start is not None and count is not None, "%s: a concatenation needs start and count" % what
        if boxes is None or boxes.numel() == 0:                      # no row anywhere: the kernel still wants an address
            if self._dummy is None:
                self._dummy = torch.zeros((1, 7), dtype=torch.float32, device=self.device)
            return self._dummy, self._block(batch, 0)[1], self._block(batch, 0)[1]
        boxes = boxes.to(device=self.device, dtype=torch.float32).contiguous()
        return boxes, start.to(device=self.device, dtype=torch.int32), count.to(device=self.device, dtype=torch.int32)

    # ---- the hot call ----------------------------------------------------------------------------------------------
    def update(self, pred, pred_start, pred_count, gt_boxes, rois=None, roi_start=None, roi_count=None, best_rcnn=None, best_roi=None,
               n_gt=None):
        """Queue one batch: the final boxes `pred` (and the first stage's `rois`; None for a one-stage model: roi_<t> stay as they
        are) against gt_boxes [B, M, ld >= 7]. Boxes come as a padded block [B, cap, ld] (start None: b * cap; count None: every
        slot, as the reference counts every slot of its zero-padded RoI block), as a concatenation [R, ld] with start / count [B],
        or as a list of per-frame tensors. Start / count tensors stay on the device. Returns nothing and waits for nothing."""
        gt = torch.as_tensor(gt_boxes)
        gt = gt.to(device=self.device, dtype=torch.float32).contiguous()
        assert gt.dim() == 3 and (gt.shape[1] == 0 or gt.shape[2] >= 7), "gt_boxes is [B, M, ld >= 7]"
        batch = gt.shape[0]
        if gt.shape[1] == 0:                                         # nothing to count (detector3d_template.py:364)
            if n_gt is not None:
                n_gt.zero_()
            return
        p, ps, pc = self._rows(pred, pred_start, pred_count, batch, "pred")
        r = rs = rc = None
        if rois is not None:
            r, rs, rc = self._rows(rois, roi_start, roi_count, batch, "rois")
        ops.recall_record(p, ps, pc, gt, self.thresh, self.counters, rois=r, roi_start=rs, roi_count=rc, best_rcnn=best_rcnn,
                          best_roi=best_roi, n_gt=n_gt)

    # ---- reading ---------------------------------------------------------------------------------------------------
    def as_dict(self):
        """The one read-back: the reference's recall_dict, Python ints, in the order the reference inserts its keys (l.353-356)."""
        got = dict(zip(self.keys, (int(v) for v in self.counters.tolist())))
        order = ["gt"] + [k % str(t) for t in self.thresh_list for k in ("roi_%s", "rcnn_%s")]
        return {k: got[k] for k in order}

    def summary(self):
        """eval_utils.py:94-101: {'recall/roi_<t>', 'recall/rcnn_<t>'} = counter / max(gt, 1)."""
        d = self.as_dict()
        gt = max(d["gt"], 1)
        out = {}
        for t in self.thresh_list:
            out["recall/roi_%s" % str(t)] = d["roi_%s" % str(t)] / gt
            out["recall/rcnn_%s" % str(t)] = d["rcnn_%s" % str(t)] / gt
        return out

    def reduce_(self, group=None):
        """Sum the counters over the ranks of `group`, in place (what merge_results_dist and the loop of eval_utils.py:75-92 do
        with the ranks' metric dicts); a no-op without a process group."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.counters, op=dist.ReduceOp.SUM, group=group)
        return self

    def load_counts(self, counts):
        """Set the counters (tests): a dict with the record's keys, or the values in counter order."""
        vals = [counts[k] for k in self.keys] if isinstance(counts, dict) else list(counts)
        assert len(vals) == len(self.keys)
        self.counters.copy_(torch.tensor([int(v) for v in vals], dtype=torch.int64))
        return self

    def reset(self):
        self.counters.zero_()
        return self


def generate_recall_record(box_preds, recall_dict, batch_index, data_dict=None, thresh_list=None):
    """Detector3DTemplate.generate_recall_record (detector3d_template.py:344-386), same arguments and return value: one frame's
    counts added to `recall_dict` (created with the reference's keys when empty). One launch and one read-back per call; a loop
    over frames that wants neither uses RecallRecord.update on the whole batch."""
    if "gt_boxes" not in data_dict:
        return recall_dict
    rois = data_dict["rois"][batch_index] if "rois" in data_dict else None
    gt = data_dict["gt_boxes"][batch_index]
    if len(recall_dict) == 0:
        recall_dict = dict([("gt", 0)] + [kv for t in thresh_list for kv in (("roi_%s" % str(t), 0), ("rcnn_%s" % str(t), 0))])
    rec = RecallRecord(thresh_list, device=box_preds.device)
    rec.update([box_preds], None, None, torch.as_tensor(gt)[None], rois=None if rois is None else [rois])
    for k, v in rec.as_dict().items():
        recall_dict[k] += v
    return recall_dict
