#!/usr/bin/env python3
"""Time the eval-time recall record (cpd_amd.recall, cpd_recall_record) on the reference's eval batch: 4 frames, 200 RoIs and the
final boxes of the shipped post-processing per frame (synthetic: about 100), about 50 ground truths per frame padded to the batch
maximum. Prints one JSON line; every figure is the median of --reps batches after --warmup:
  a_reference_loop_ms   generate_recall_record as the reference writes it (detector3d_template.py:344-386), frame by frame on the
                        operators the library had before this one: boxes_iou3d_gpu, max, `.item()` per threshold and side, the
                        trimming loop with its host test per row; host clock, device synchronised at the end
  b_update_as_dict_ms   RecallRecord.update for the batch + one as_dict() (the one read-back); host clock
  c_update_event_ms     the update alone, from HIP events
  d_engine_ms / d_engine_recall_ms   the fused two-stage engine step (cpd_amd.two_stage, the benchmark's model and 4 synthetic
                        frames) without and with a record attached; host clock, device synchronised at the end
Not part of bench.py. Usage: python tools/recall_time.py [--reps 20] [--warmup 5] [--no-engine]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import iou3d_nms_utils, recall  # noqa: E402

THRESH = [0.3, 0.5, 0.7]


def reference_loop(final_boxes, recall_dict, batch_index, data_dict, thresh_list):
    """The reference's method, statement for statement, on this library's boxes_iou3d_gpu."""
    rois = data_dict['rois'][batch_index] if 'rois' in data_dict else None
    gt_boxes = data_dict['gt_boxes'][batch_index]
    if len(recall_dict) == 0:
        recall_dict = {'gt': 0}
        for t in thresh_list:
            recall_dict['roi_%s' % str(t)] = 0
            recall_dict['rcnn_%s' % str(t)] = 0
    cur_gt = gt_boxes
    k = len(cur_gt) - 1
    while k > 0 and cur_gt[k].sum() == 0:
        k -= 1
    cur_gt = cur_gt[:k + 1]
    if cur_gt.shape[0] > 0:
        iou_rcnn = iou3d_nms_utils.boxes_iou3d_gpu(final_boxes[:, 0:7], cur_gt[:, 0:7]) if final_boxes.shape[0] > 0 else None
        iou_roi = iou3d_nms_utils.boxes_iou3d_gpu(rois[:, 0:7], cur_gt[:, 0:7]) if rois is not None else None
        for t in thresh_list:
            if iou_rcnn is not None:
                recall_dict['rcnn_%s' % str(t)] += (iou_rcnn.max(dim=0)[0] > t).sum().item()
            if iou_roi is not None:
                recall_dict['roi_%s' % str(t)] += (iou_roi.max(dim=0)[0] > t).sum().item()
        recall_dict['gt'] += cur_gt.shape[0]
    return recall_dict


def synthetic_batch(seed, frames=4, n_roi=200):
    rng = np.random.default_rng(seed)

    def boxes(n):
        b = np.zeros((n, 7), np.float32)
        b[:, :2] = rng.uniform(-70, 70, (n, 2))
        b[:, 2] = rng.uniform(-1, 1, n)
        b[:, 3:6] = np.exp(rng.normal(0, 0.2, (n, 3))) * np.array([4.7, 2.1, 1.7])
        b[:, 6] = rng.uniform(-np.pi, np.pi, n)
        return b

    def near(gt, n, s):
        src = gt[rng.integers(0, len(gt), n)].astype(np.float64)
        src[:, :2] += rng.normal(0, 1.0, (n, 2)) * s
        src[:, 3:6] *= np.exp(rng.normal(0, 0.1, (n, 3)))
        src[:, 6] += rng.normal(0, 0.2, n) * s
        return src.astype(np.float32)

    gts, rois, finals = [], np.zeros((frames, n_roi, 7), np.float32), []
    for f in range(frames):
        g = boxes(int(rng.integers(40, 61)))
        gts.append(np.concatenate([g, rng.integers(1, 4, (len(g), 1)).astype(np.float32)], axis=1))
        n_real = n_roi - int(rng.integers(0, 30))                        # zero-padded slots behind the frame's own RoIs
        rois[f, :n_real] = np.concatenate([near(g, n_real - 60, 0.8), boxes(60)])
        finals.append(np.concatenate([near(g, int(rng.integers(70, 110)), 0.4), boxes(20)]))
    return finals, rois, recall.pad_gt(gts)


def median_ms(fn, reps, warmup):
    out = []
    for i in range(reps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(out)), 4)


def engine_times(reps, warmup):
    from cpd_amd import models
    from cpd_amd.engine import ModelConfig, init_state_dict
    from cpd_amd.synthetic import waymo_cloud
    from cpd_amd.two_stage import VoxelRCNNEngine
    cfg = ModelConfig()
    sd = init_state_dict(cfg, 0)
    mcfg = models.waymo_voxel_rcnn_cfg()
    torch.manual_seed(0)
    head = models.__all__[mcfg.ROI_HEAD.NAME](input_channels={"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 128},
                                              model_cfg=mcfg.ROI_HEAD, point_cloud_range=cfg.point_cloud_range, voxel_size=cfg.voxel_size,
                                              num_class=1)
    with torch.no_grad():
        head.cls_layers[-1].weight.normal_(0, 0.3); head.cls_layers[-1].bias.normal_(0, 0.3)
        head.reg_layers[-1].weight.normal_(0, 0.01); head.reg_layers[-1].bias.zero_()
    sd.update({"roi_head." + k: v.detach().clone() for k, v in head.state_dict().items()})
    eng = VoxelRCNNEngine(cfg, mcfg.ROI_HEAD, mcfg.POST_PROCESSING, sd)
    clouds = [torch.from_numpy(waymo_cloud(s)).cuda() for s in range(4)]
    out, it = eng.forward(clouds, return_intermediates=True)
    gts = []
    for b in range(4):                                                   # about 50 gts per frame next to the frame's own RoIs
        r = it["rois"][b].cpu()
        r = r[r[:, 3] > 0]
        r = r[torch.randperm(len(r), generator=torch.Generator().manual_seed(b))[:50 + 3 * b], :7].clone()
        r[:, :2] += 0.1 * r[:, 3:5]
        gts.append(torch.cat([r, torch.ones(len(r), 1)], dim=1))
    gt = recall.pad_gt(gts).cuda()
    rec = recall.RecallRecord(THRESH)
    plain = median_ms(lambda: eng.forward(clouds), reps, warmup)
    with_rec = median_ms(lambda: eng.forward(clouds, gt_boxes=gt, recall=rec), reps, warmup)
    return {"d_engine_ms": plain, "d_engine_recall_ms": with_rec, "engine_rois": int(it["rois"].shape[1]),
            "engine_final_boxes": [int(len(o["pred_boxes"])) for o in out], "engine_gt_cap": int(gt.shape[1]),
            "engine_record": rec.as_dict()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    finals, rois, gt = synthetic_batch(1)
    finals = [torch.from_numpy(f).cuda() for f in finals]
    rois, gt = torch.from_numpy(rois).cuda(), gt.cuda()
    data = {"rois": rois, "gt_boxes": gt}
    batch = len(finals)

    def loop():
        d = {}
        for b in range(batch):
            d = reference_loop(finals[b], d, b, data, THRESH)
        return d

    rec = recall.RecallRecord(THRESH)

    def fused():
        rec.reset()
        rec.update(finals, None, None, gt, rois=rois)
        return rec.as_dict()

    assert loop() == fused(), (loop(), fused())
    line = {"frames": batch, "rois": int(rois.shape[1]), "final_boxes": [int(len(f)) for f in finals], "gt_cap": int(gt.shape[1]),
            "record": fused(), "reps": args.reps, "warmup": args.warmup}
    line["a_reference_loop_ms"] = median_ms(loop, args.reps, args.warmup)
    line["b_update_as_dict_ms"] = median_ms(fused, args.reps, args.warmup)
    # (c) the launch alone: a padded block and its device counts, as the engine hands them over
    cap = max(len(f) for f in finals)
    blk = torch.zeros((batch, cap, 7), device="cuda")
    for b, f in enumerate(finals):
        blk[b, :len(f)] = f
    cnt = torch.tensor([len(f) for f in finals], dtype=torch.int32, device="cuda")
    ev = []
    for i in range(args.reps + args.warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rec.update(blk, None, cnt, gt, rois=rois)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ev.append(e0.elapsed_time(e1))
    line["c_update_event_ms"] = round(float(np.median(ev)), 4)
    if not args.no_engine:
        line.update(engine_times(args.reps, args.warmup))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
