#!/usr/bin/env python3
"""Times the anchor-head VoxelRCNN's RoI-head training on one GPU (numbers quoted in DESIGN.md):
  * get_loss: the fused `cpd_rcnn_loss` (roi_head_train.rcnn_head_loss: one launch + the tb_dict read-back) against the torch
    restatement rcnn_head_loss_torch (+ its .item() read-backs), at the shipped size B = 2, ROI_PER_IMAGE = 150, with backward;
  * one head training step: forward (proposal layer, sampling, pooling, FC stacks) + get_loss + backward, the shipped ROI_HEAD of
    voxel_rcnn_dbscan_single_train.yaml (GRID_SIZE 6; x_conv3 / x_conv4 with two radii each: four pooling scales) on synthetic
    sparse levels and proposals; the same step split into phases by events (proposal layer, target sampling, pooling forward, FC
    stacks, loss, backward) and its peak allocated memory. --fused-pool turns NeighborVoxelSAModuleMSG.fused_train on
    (roi_pool.set_fused_train): pooling through cpd_voxel_pool_max_train instead of the module sequence.
  * the head step and its "target sampling" phase with ProposalTargetLayer.fused off (the torch path) and on (cpd_roi_targets_classify /
    cpd_roi_targets_gather: two launches, one read-back, one upload), alternated in one process --pairs times: per-pair medians and
    the overall ones.
Median of cuda-event-timed repetitions after warm-up. Prints one JSON line.
Usage: python tools/rcnn_head_train_time.py [--fused-pool] [--pairs 5]"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps=50, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def loss_rows(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    rois = torch.cat([(r(n, 2) - 0.5) * 60, r(n, 1) - 0.5, 0.6 + 4 * r(n, 3), (r(n, 1) - 0.5) * 6.4], 1)
    gt = torch.cat([torch.randn(n, 3, generator=g) * 0.4, rois[:, 3:6] * (0.8 + 0.4 * r(n, 3)), (r(n, 1) - 0.5) * 3, torch.ones(n, 1)], 1)
    src = torch.cat([rois[:, 0:3] + torch.randn(n, 3, generator=g) * 0.4, gt[:, 3:6], rois[:, 6:7], torch.ones(n, 1)], 1)
    t = dict(rcnn_cls=torch.randn(n, 1, generator=g), rcnn_reg=torch.randn(n, 7, generator=g) * 0.3, rois=rois.view(2, -1, 7),
             gt_of_rois=gt.view(2, -1, 8), gt_of_rois_src=src.view(2, -1, 8), reg_valid_mask=(r(n) < 0.5).long().view(2, -1),
             rcnn_cls_labels=r(n).view(2, -1))
    return {k: v.cuda() for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fused-pool", action="store_true", help="train the pooling through the fused op (fused_train on every pooling module)")
    ap.add_argument("--pairs", type=int, default=5, help="how many times the two target-layer settings are alternated")
    opt = ap.parse_args()
    from cpd_amd import models, roi_pool
    from cpd_amd.roi_head_train import assign_targets, set_fused_targets
    from cpd_amd.roi_head_train import rcnn_head_loss, rcnn_head_loss_torch
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0)}
    cfg = models.waymo_voxel_rcnn_dbscan_cfg().ROI_HEAD
    per = int(cfg.TARGET_CONFIG["ROI_PER_IMAGE"])
    n = 2 * per
    t = loss_rows(n)
    lw = cfg.LOSS_CONFIG["LOSS_WEIGHTS"]
    w = (lw["code_weights"], lw["rcnn_cls_weight"], lw["rcnn_reg_weight"], lw["rcnn_corner_weight"], True)
    cls, reg = t["rcnn_cls"].requires_grad_(True), t["rcnn_reg"].requires_grad_(True)
    args = (cls, reg, t["rois"], t["gt_of_rois"], t["gt_of_rois_src"], t["reg_valid_mask"], t["rcnn_cls_labels"])

    def fused():
        loss, losses = rcnn_head_loss(*args, *w)
        losses.tolist()                                              # the tb_dict read-back of VoxelRCNNHead.get_loss
        loss.backward()

    def restated():
        loss, terms = rcnn_head_loss_torch(*args, *w)
        [v.item() for k, v in terms.items() if k != "fg"]            # the reference's .item() calls
        loss.backward()
    out["get_loss_rows"] = n
    out["get_loss_fused_ms"] = timed(fused)
    out["get_loss_torch_ms"] = timed(restated)

    # one head training step at the shipped ROI_HEAD
    chans = {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 128}
    pcr = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
    vs = [0.1, 0.1, 0.15]
    torch.manual_seed(0)
    head = roi_pool.VoxelRCNNHead(chans, cfg, point_cloud_range=pcr, voxel_size=vs, num_class=1).cuda().train()
    head.init_weights()
    out["fused_pool"] = bool(opt.fused_pool)
    if opt.fused_pool:
        roi_pool.set_fused_train(head)
    rng = np.random.default_rng(0)
    B, n_gt = 2, 40
    gt = np.zeros((B, n_gt, 8), np.float32)
    gt[..., 0:2] = rng.uniform(-60, 60, (B, n_gt, 2))
    gt[..., 2] = rng.uniform(-0.5, 0.5, (B, n_gt))
    gt[..., 3:6] = [4.5, 2.0, 1.6]
    gt[..., 6] = rng.uniform(-3, 3, (B, n_gt))
    gt[..., 7] = 1
    boxes = np.repeat(gt[:, :, None, :7], 100, 2)
    boxes[..., 0:3] += rng.normal(0, 0.4, boxes[..., 0:3].shape)
    boxes = boxes.reshape(B, -1, 7).astype(np.float32)
    scores = rng.normal(0, 1, (B, boxes.shape[1], 3)).astype(np.float32)
    levels = {}
    for name, stride, nvox in (("x_conv3", 4, 60000), ("x_conv4", 8, 20000)):
        shp = [41 // stride + 1, 1504 // stride, 1504 // stride]
        idx = np.stack([rng.integers(0, B, nvox), rng.integers(0, shp[0], nvox), rng.integers(0, shp[1], nvox), rng.integers(0, shp[2], nvox)], 1)
        idx = torch.from_numpy(np.unique(idx, axis=0).astype(np.int32)).cuda()
        f = torch.randn(idx.shape[0], chans[name], device="cuda").requires_grad_(True)
        levels[name] = types.SimpleNamespace(indices=idx, features=f, spatial_shape=shp, batch_size=B)
    gt_t, boxes_t, scores_t = torch.from_numpy(gt).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()

    def batch():
        return {"batch_size": B, "batch_box_preds": boxes_t, "batch_cls_preds": scores_t, "gt_boxes": gt_t, "multi_scale_3d_features": levels,
                "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}

    def step():
        bd = batch()
        head(bd)
        loss, _ = head.get_loss()
        head.zero_grad(set_to_none=True)
        loss.backward()
    out["head_step_rois"] = B * per
    out["head_step_ms"] = timed(step, reps=20, warmup=3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    out["head_step_peak_mb"] = torch.cuda.max_memory_allocated() / 2 ** 20

    # the same step, VoxelRCNNHead.forward's training branch statement by statement with an event between the phases
    names = ("proposal_layer", "target_sampling", "pooling_forward", "fc_stacks", "loss", "backward")

    def phases():
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        bd = batch()
        marks[0].record()
        head._fc = None
        head._proposals(bd, "TRAIN")
        marks[1].record()
        targets = assign_targets(head.proposal_target_layer, bd)
        bd["rois"], bd["roi_labels"] = targets["rois"], targets["roi_labels"]
        marks[2].record()
        pooled = head._pool(bd)
        marks[3].record()
        shared = head.shared_fc_layers(pooled.reshape(pooled.shape[0], -1))
        targets.update(rcnn_cls=head.cls_layers(shared), rcnn_reg=head.reg_layers(shared))
        head.forward_ret_dict = targets
        marks[4].record()
        loss, _ = head.get_loss()
        marks[5].record()
        head.zero_grad(set_to_none=True)
        loss.backward()
        marks[6].record()
        marks[6].synchronize()
        return [marks[i].elapsed_time(marks[i + 1]) for i in range(len(names))]
    for _ in range(3):
        phases()
    runs = np.array([phases() for _ in range(20)])
    out["head_step_phases_ms"] = {k: float(v) for k, v in zip(names, np.median(runs, axis=0))}

    # the device target layer against the torch path: the settings alternated, the "target sampling" phase and the whole step
    per_pair = {key: {"target_sampling": [], "head_step": []} for key in ("torch", "fused")}
    every = {key: {"target_sampling": [], "head_step": []} for key in ("torch", "fused")}
    for _ in range(opt.pairs):
        for key, flag in (("torch", False), ("fused", True)):
            set_fused_targets(head, flag)
            phases()
            sampling = [phases()[1] for _ in range(20)]
            steps = []
            step()
            torch.cuda.synchronize()
            for _ in range(10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step()
                b.record()
                b.synchronize()
                steps.append(a.elapsed_time(b))
            for name, t in (("target_sampling", sampling), ("head_step", steps)):
                per_pair[key][name].append(float(np.median(t)))
                every[key][name] += t
    set_fused_targets(head, False)
    out["fused_targets"] = {"pairs": opt.pairs}
    for name in ("target_sampling", "head_step"):
        out["fused_targets"][name] = {
            "torch_ms": float(np.median(every["torch"][name])), "fused_ms": float(np.median(every["fused"][name])),
            "pairs_torch_ms": per_pair["torch"][name], "pairs_fused_ms": per_pair["fused"][name],
            "fused_below_torch_in_every_pair": all(f < t for f, t in zip(per_pair["fused"][name], per_pair["torch"][name]))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
