#!/usr/bin/env python3
"""Times the prototype RoI head's training on one GPU, at the shipped ROI_HEAD of voxel_rcnn_cproto_center.yaml (B = 4, ROI_PER_IMAGE =
130: 520 rows, shared features 256 wide; GRID_SIZE 6, both pooling branches) -- numbers quoted in DESIGN.md:
  * get_loss + backward + the tb_dict read-back on synthetic targets_dict0 / targets_dict1: VoxelRCNNProtoHead.fused_loss on (one
    `cpd_rcnn_proto_loss` launch) against off (the torch chain with its read-backs);
  * one head training step -- forward (proposal layer, sampling, both pooling branches with fused_train on, FC stacks) + get_loss +
    backward on synthetic sparse levels and proposals -- with fused_loss off and on, and the same step split into phases by events;
  * with fused_loss on, the head step and its "target sampling" phase with ProposalTargetLayer.fused off (the torch path) and on
    (cpd_roi_targets_classify / cpd_roi_targets_gather: two launches, one read-back, one upload).
The two settings of a switch are alternated in one process, --pairs times; every figure is the median of event-timed repetitions after warm-up,
per pair and over all pairs. Prints one JSON line.  Usage: python tools/proto_head_train_time.py [--pairs 5]"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup):
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
    return out


def alternated(run, pairs, reps, warmup):
    """run(fused) timed `reps` times with fused_loss off, then on, `pairs` times over -> the per-pair medians and the overall ones."""
    per = {"torch": [], "fused": []}
    every = {"torch": [], "fused": []}
    for _ in range(pairs):
        for key, flag in (("torch", False), ("fused", True)):
            t = timed(lambda: run(flag), reps, warmup)
            per[key].append(float(np.median(t)))
            every[key] += t
    return {"torch_ms": float(np.median(every["torch"])), "fused_ms": float(np.median(every["fused"])), "pairs_torch_ms": per["torch"],
            "pairs_fused_ms": per["fused"], "fused_below_torch_in_every_pair": all(f < t for f, t in zip(per["fused"], per["torch"]))}


def loss_targets(b, per, width, seed=0):
    """targets_dict0 / targets_dict1 as VoxelRCNNProtoHead.forward leaves them, on synthetic rows."""
    n = b * per
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    rois = torch.cat([(r(n, 2) - 0.5) * 60, r(n, 1) - 0.5, 0.6 + 4 * r(n, 3), (r(n, 1) - 0.5) * 6.4], 1)
    gt = torch.cat([torch.randn(n, 3, generator=g) * 0.4, rois[:, 3:6] * (0.8 + 0.4 * r(n, 3)), (r(n, 1) - 0.5) * 3, torch.ones(n, 1)], 1)
    src = torch.cat([rois[:, 0:3] + torch.randn(n, 3, generator=g) * 0.4, gt[:, 3:6], rois[:, 6:7], torch.ones(n, 1)], 1)
    shared = dict(rois=rois.view(b, per, 7), gt_of_rois=gt.view(b, per, 8), gt_of_rois_src=src.view(b, per, 8),
                  reg_valid_mask=(r(n) < 0.5).long().view(b, per), rcnn_cls_labels=r(n).view(b, per))
    css = torch.where(r(n) < 0.2, torch.zeros(n), 0.2 + 0.8 * r(n)).view(b, per)
    ts = []
    for _ in (0, 1):
        t = {k: v.clone().cuda() for k, v in shared.items()}
        t["additional_data"] = {"css_score": css.clone().cuda()}
        t.update(rcnn_cls=torch.randn(n, 1, generator=g).cuda().requires_grad_(True), rcnn_reg=(torch.randn(n, 7, generator=g) * 0.3).cuda().requires_grad_(True),
                 shared_features=torch.relu(torch.randn(n, width, generator=g)).cuda().requires_grad_(True))
        ts.append(t)
    return ts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=5, help="how many times the two settings are alternated")
    opt = ap.parse_args()
    from cpd_amd import models, roi_pool
    from cpd_amd.roi_head_train import VoxelRCNNProtoHead, assign_targets, set_fused_targets
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "pairs": opt.pairs}
    cfg = models.waymo_voxel_rcnn_cfg().ROI_HEAD
    B, per, width = 4, int(cfg.TARGET_CONFIG["ROI_PER_IMAGE"]), int(cfg.SHARED_FC[-1])
    chans = {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 128}
    pcr, vs = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0], [0.1, 0.1, 0.15]
    torch.manual_seed(0)
    head = VoxelRCNNProtoHead(chans, cfg, point_cloud_range=pcr, voxel_size=vs, num_class=1).cuda().train()
    roi_pool.set_fused_train(head)

    # get_loss + backward + the read-back
    t0, t1 = loss_targets(B, per, width)
    head.forward_ret_dict = {"targets_dict0": t0, "targets_dict1": t1}

    def get_loss(fused):
        head.fused_loss = fused
        loss, tb = head.get_loss()                                   # (tb_dict["rcnn_loss"] is the read-back; the torch path makes ~10)
        loss.backward()
    out["get_loss_rows"], out["get_loss_feat_dim"] = B * per, width
    out["get_loss"] = alternated(get_loss, opt.pairs, reps=30, warmup=5)

    # one head training step
    rng = np.random.default_rng(0)
    n_gt = 40
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
    css = rng.uniform(0.2, 1.0, (B, n_gt)).astype(np.float32)
    css[:, ::5] = 0.0
    levels, levels_mm = {}, {}
    for name, stride, nvox in (("x_conv3", 4, 120000), ("x_conv4", 8, 40000)):
        shp = [41 // stride + 1, 1504 // stride, 1504 // stride]
        idx = np.stack([rng.integers(0, B, nvox), rng.integers(0, shp[0], nvox), rng.integers(0, shp[1], nvox), rng.integers(0, shp[2], nvox)], 1)
        idx = torch.from_numpy(np.unique(idx, axis=0).astype(np.int32)).cuda()
        for d in (levels, levels_mm):
            f = torch.randn(idx.shape[0], chans[name], device="cuda").requires_grad_(True)
            d[name] = types.SimpleNamespace(indices=idx, features=f, spatial_shape=shp, batch_size=B)
    gt_t, boxes_t, scores_t, css_t = (torch.from_numpy(a).cuda() for a in (gt, boxes, scores, css))

    def batch():
        return {"batch_size": B, "batch_box_preds": boxes_t, "batch_cls_preds": scores_t, "gt_boxes": gt_t, "css_score": css_t,
                "multi_scale_3d_features": levels, "multi_scale_3d_features_mm": levels_mm, "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}

    def step(fused):
        head.fused_loss = fused
        head(batch())
        loss, _ = head.get_loss()
        head.zero_grad(set_to_none=True)
        loss.backward()
    out["head_step_rois"] = B * per
    out["head_step"] = alternated(step, opt.pairs, reps=10, warmup=2)

    # the same step, VoxelRCNNProtoHead.forward's training branch statement by statement with an event between the phases (both
    # pooling branches first, then the FC stacks: the same work as forward's pool / FC / pool / FC order)
    names = ("proposal_layer", "target_sampling", "pooling_forward", "fc_stacks", "loss", "backward")

    def phases(fused):
        head.fused_loss = fused
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        bd = batch()
        marks[0].record()
        head.proposal_layer(bd, cfg.NMS_CONFIG["TRAIN"])
        marks[1].record()
        targets = assign_targets(head.proposal_target_layer, bd)
        bd["rois"], bd["roi_labels"] = targets["rois"], targets["roi_labels"]
        copy = lambda t: {k: ({kk: vv.clone() for kk, vv in v.items()} if k == "additional_data" else v.clone()) for k, v in t.items()}
        u0, u1 = copy(targets), copy(targets)
        marks[2].record()
        pooled, pooled_p = head.roi_grid_pool(bd), head.roi_grid_pool_mm(bd)
        marks[3].record()
        shared = head.shared_fc_layers(pooled.reshape(pooled.shape[0], -1))
        u0.update(rcnn_cls=head.cls_layers(shared), rcnn_reg=head.reg_layers(shared), shared_features=shared)
        shared_p = head.shared_fc_layers_mm(pooled_p.reshape(pooled_p.shape[0], -1))
        u1.update(rcnn_cls=head.cls_layers_P(shared_p), rcnn_reg=head.reg_layers_P(shared_p), shared_features=shared_p)
        head.forward_ret_dict = {"targets_dict0": u0, "targets_dict1": u1}
        marks[4].record()
        loss, _ = head.get_loss()
        marks[5].record()
        head.zero_grad(set_to_none=True)
        loss.backward()
        marks[6].record()
        marks[6].synchronize()
        return [marks[i].elapsed_time(marks[i + 1]) for i in range(len(names))]
    runs = {False: [], True: []}
    for flag in (False, True):
        for _ in range(2):
            phases(flag)
    for _ in range(opt.pairs):
        for flag in (False, True):
            runs[flag] += [phases(flag) for _ in range(10)]
    out["head_step_phases_ms"] = {key: {k: float(v) for k, v in zip(names, np.median(np.array(runs[flag]), axis=0))}
                                  for key, flag in (("torch", False), ("fused", True))}

    # the device target layer against the torch path (fused_loss on in both settings)
    def step_targets(fused_targets):
        set_fused_targets(head, fused_targets)
        step(True)

    def sampling(fused_targets):
        set_fused_targets(head, fused_targets)
        return phases(True)[1]
    for flag in (False, True):
        sampling(flag)
    per, every = {"torch": [], "fused": []}, {"torch": [], "fused": []}
    for _ in range(opt.pairs):
        for key, flag in (("torch", False), ("fused", True)):
            sampling(flag)
            t = [sampling(flag) for _ in range(20)]
            per[key].append(float(np.median(t)))
            every[key] += t
    out["fused_targets"] = {
        "target_sampling": {"torch_ms": float(np.median(every["torch"])), "fused_ms": float(np.median(every["fused"])),
                            "pairs_torch_ms": per["torch"], "pairs_fused_ms": per["fused"],
                            "fused_below_torch_in_every_pair": all(f < t for f, t in zip(per["fused"], per["torch"]))},
        "head_step": alternated(step_targets, opt.pairs, reps=10, warmup=2)}
    set_fused_targets(head, False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
