#!/usr/bin/env python3
"""Golden vectors of the eval-time recall record (tests/golden/recall.npz). Only DATA is written.

What runs here is the reference's own Detector3DTemplate.generate_recall_record
(cpd/models/detectors/detector3d_template.py:344-386), loaded from the reference tree by file path under the synthetic package
`r` of make_golden.py with its missing siblings as empty modules; its iou3d_nms_utils.boxes_iou3d_gpu is the oracle's
boxes_iou3d on host tensors. Should the module not import (it pulls in every model package), the method's source is read
from that file at maker time and executed on its own: the text is never stored.

Cases (thresholds [0.3, 0.5, 0.7]; every case is a sequence of frames fed to ONE dict, the dict recorded after every frame):
  plain_*   two-stage, 4 frames, gt block [4, 12, 8]: 9 of 12 rows real; 12 real rows with an interior zero row; 7 real rows, a
            trailing row [1, -1, 0, ...] (sums to zero: trimmed) and zero rows; a frame without predictions. RoI blocks
            [4, R, 7] with zero-padded slots.
  one_*     the same frames without rois (one-stage: the roi counters stay 0).
  zero_*    an all-zero gt block [1, 5, 8]: one gt counted, never recalled.
  empty_*   gt_cap == 0 ([1, 0, 8]): nothing counted.
  twice_*   two successive batches on one dict (plain's frames, then 2 frames of another seed, gt block [2, 12, 8]).
Per case X: X_pred [sum n, 7] + X_pred_n [B] (the frames' final boxes, concatenated), X_rois [B, R, 7] (two-stage only),
X_gt [B, M, 8], X_dicts [B, 7] (the dict after each frame, in the order gt, roi_<t> .., rcnn_<t> ..), and from the oracle's
IoU matrices X_best_rcnn / X_best_roi [B, M] (the column maxima the counters were taken from, -1 for rows not counted or
without boxes) and X_ngt [B].
Asserted here: every counted gt's best IoU lies at least 1e-3 from every threshold (the device IoU contract is 1e-4), and in
the plain case each of the six recall counters lies strictly between 0 and gt.
Usage:  python tests/golden/make_golden_recall.py
"""
import os
import re
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
import ref_recall as R  # noqa: E402
from oracle import Oracle  # noqa: E402

THRESH = [0.3, 0.5, 0.7]
REL = "cpd/models/detectors/detector3d_template.py"


def load_reference_method(oracle):
    iou_mod = types.ModuleType("r.ops.iou3d_nms.iou3d_nms_utils")

    def boxes_iou3d_gpu(a, b):
        return torch.from_numpy(oracle.boxes_iou3d(np.ascontiguousarray(a.numpy(), np.float32), np.ascontiguousarray(b.numpy(), np.float32)))

    iou_mod.boxes_iou3d_gpu = boxes_iou3d_gpu
    try:
        for p in ["r", "r.models", "r.models.detectors", "r.utils", "r.ops", "r.ops.iou3d_nms", "r.models.backbones_2d", "r.models.backbones_3d",
                  "r.models.dense_heads", "r.models.roi_heads", "r.models.wrap_head", "r.models.backbones_2d.map_to_bev",
                  "r.models.temporal_model", "r.models.temporal_model.temporal_model", "r.models.backbones_3d.pfe",
                  "r.models.backbones_3d.vfe", "r.models.model_utils", "r.models.model_utils.model_nms_utils"]:
            MG._pkg(p)
        su = types.ModuleType("r.utils.spconv_utils")
        su.find_all_spconv_keys = lambda *a, **k: set()
        sys.modules["r.utils.spconv_utils"] = su
        sys.modules["r.ops.iou3d_nms.iou3d_nms_utils"] = iou_mod
        sys.modules["r.ops.iou3d_nms"].iou3d_nms_utils = iou_mod
        mod = MG._load("r.models.detectors.detector3d_template", REL)
        print("reference class imported")
        return mod.Detector3DTemplate.generate_recall_record
    except Exception as e:                                   # the method alone, from the file's text
        print("class import failed (%s): executing the method's source" % e)
        text = open(os.path.join(MG.REF, REL)).read()
        m = re.search(r"^    @staticmethod\n(    def generate_recall_record\(.*?)(?=^    def )", text, re.S | re.M)
        ns = {"torch": torch, "iou3d_nms_utils": iou_mod}
        exec(textwrap.dedent(m.group(1)), ns)
        return ns["generate_recall_record"]


def rand_gt(rng, n):
    """n boxes on a jittered grid: none overlaps another"""
    cells = rng.permutation(36)[:n]
    b = np.zeros((n, 8), np.float32)
    b[:, 0] = (cells % 6) * 12.0 - 30.0 + rng.uniform(-1, 1, n)
    b[:, 1] = (cells // 6) * 12.0 - 30.0 + rng.uniform(-1, 1, n)
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3:6] = np.exp(rng.normal(0, 0.2, (n, 3))) * np.array([4.7, 2.1, 1.7])
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    b[:, 7] = rng.integers(1, 4, n)
    return b


def jittered(rng, gt, scales):
    """one box per gt row and scale: the gt moved / resized / turned by a scale-sized amount (IoUs from about 0.9 down to 0)"""
    out = []
    for g in gt:
        for s in scales:
            b = g[:7].astype(np.float64).copy()
            b[:2] += rng.normal(0, 1.0, 2) * s * 2.0
            b[2] += rng.normal(0, 0.3) * s
            b[3:6] *= np.exp(rng.normal(0, 0.25, 3) * s)
            b[6] += rng.normal(0, 0.4) * s
            out.append(b)
    return np.array(out, np.float32).reshape(-1, 7)


def make_frames(seed, shapes, cap=12):
    """shapes: list of (kind, n_real). -> preds (list), rois (list), gt block [B, cap, 8]"""
    rng = np.random.default_rng(seed)
    preds, rois, gts = [], [], np.zeros((len(shapes), cap, 8), np.float32)
    for f, (kind, n) in enumerate(shapes):
        g = rand_gt(rng, n)
        gts[f, :n] = g
        real = g
        if kind == "interior":
            gts[f, 4] = 0                                    # a zero row between real rows: counted, never recalled
            real = np.delete(g, 4, axis=0)
        if kind == "cancel":
            gts[f, n] = 0
            gts[f, n, 0], gts[f, n, 1] = 1.0, -1.0           # sums to zero in any order of addition: trimmed
        s_pred = rng.choice([0.05, 0.15, 0.3, 0.5, 0.8], len(real))
        s_roi = rng.choice([0.1, 0.25, 0.45, 0.7, 1.0], len(real))
        p = np.concatenate([jittered(rng, real[i:i + 1], [s_pred[i]]) for i in range(len(real))] + [rand_gt(rng, 3)[:, :7]])
        r = np.concatenate([jittered(rng, real[i:i + 1], [s_roi[i], 1.5 * s_roi[i]]) for i in range(len(real))] + [rand_gt(rng, 4)[:, :7]])
        if kind == "nopred":
            p = np.zeros((0, 7), np.float32)
        preds.append(p[rng.permutation(len(p))])
        rois.append(r[rng.permutation(len(r))])
    return preds, rois, gts


def roi_block(rois):
    out = np.zeros((len(rois), max(len(r) for r in rois) + 2, 7), np.float32)      # every frame keeps zero-padded slots
    for f, r in enumerate(rois):
        out[f, :len(r)] = r
    return out


def run_case(method, oracle, preds, rois_blk, gts, start=None):
    """the reference's method over the frames on one dict -> (dicts [B, 7], best_rcnn, best_roi, n_gt)"""
    keys = R.record_keys(THRESH)
    data = {"gt_boxes": torch.from_numpy(gts)}
    if rois_blk is not None:
        data["rois"] = torch.from_numpy(rois_blk)
    d = dict(start or {})
    dicts = []
    for f in range(len(gts)):
        d = method(box_preds=torch.from_numpy(preds[f]), recall_dict=d, batch_index=f, data_dict=data, thresh_list=THRESH)
        dicts.append([int(d[k]) for k in keys])
    total, br, bo, ng = R.batch_record(oracle, preds, gts, rois_blk, THRESH)
    for best in (br, bo):                                    # the margin every exact-count test relies on
        counted = best[best >= 0]
        for t in THRESH:
            assert counted.size == 0 or np.abs(counted - t).min() >= 1e-3, "a best IoU within 1e-3 of %.1f" % t
    return np.array(dicts, np.int64).reshape(len(gts), len(keys)), br, bo, ng, d


def store(out, name, preds, rois_blk, gts, res):
    out[name + "_pred"] = np.concatenate(preds).astype(np.float32).reshape(-1, 7)
    out[name + "_pred_n"] = np.array([len(p) for p in preds], np.int32)
    if rois_blk is not None:
        out[name + "_rois"] = rois_blk
    out[name + "_gt"] = gts
    out[name + "_dicts"], out[name + "_best_rcnn"], out[name + "_best_roi"], out[name + "_ngt"] = res[:4]


def main():
    oracle = Oracle()
    method = load_reference_method(oracle)
    shapes = [("plain", 9), ("interior", 12), ("cancel", 7), ("nopred", 6)]
    out = {"thresh": np.array(THRESH, np.float64), "keys": np.array(R.record_keys(THRESH))}
    for seed in range(20261019, 20261019 + 200):
        try:
            preds, rois, gts = make_frames(seed, shapes)
            blk = roi_block(rois)
            plain = run_case(method, oracle, preds, blk, gts)
            last = plain[0][-1]
            assert all(0 < v < last[0] for v in last[1:]), "a recall counter at 0 or at gt: %s" % last
            one = run_case(method, oracle, preds, None, gts)
            p2, r2, g2 = make_frames(seed + 5000, [("plain", 11), ("plain", 5)])
            twice = run_case(method, oracle, p2, roi_block(r2), g2, start=plain[4])
        except AssertionError as e:
            print("seed %d rejected: %s" % (seed, e))
            continue
        print("seed %d" % seed)
        break
    else:
        raise RuntimeError("no seed meets the conditions")
    assert list(plain[3]) == [9, 12, 7, 6]
    assert all(v == 0 for v in one[0][-1][1:4]) and list(one[0][-1][4:]) == list(plain[0][-1][4:])
    store(out, "plain", preds, blk, gts, plain)
    store(out, "one", preds, None, gts, one)
    store(out, "twice", p2, roi_block(r2), g2, twice)
    rng = np.random.default_rng(7)
    zp, zr, zg = [rand_gt(rng, 4)[:, :7]], np.zeros((1, 3, 7), np.float32), np.zeros((1, 5, 8), np.float32)
    zr[0, :2] = rand_gt(rng, 2)[:, :7]
    zero = run_case(method, oracle, zp, zr, zg)
    assert list(zero[0][-1]) == [1, 0, 0, 0, 0, 0, 0]
    store(out, "zero", zp, zr, zg, zero)
    eg = np.zeros((1, 0, 8), np.float32)
    empty = run_case(method, oracle, zp, zr, eg)
    assert list(empty[0][-1]) == [0] * 7
    store(out, "empty", zp, zr, eg, empty)
    path = os.path.join(HERE, "recall.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    for name in ("plain", "one", "twice", "zero", "empty"):
        print(name, dict(zip(R.record_keys(THRESH), out[name + "_dicts"][-1])))


if __name__ == "__main__":
    main()
