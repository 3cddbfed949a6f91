#!/usr/bin/env python3
"""Golden vectors of the anchor-head VoxelRCNN's RoI-head training (run in the build container only, like make_golden.py, whose
loaders it imports): the REFERENCE's own code, loaded by file path, on CPU.

  voxel_rcnn_head_train.npz  VoxelRCNNHead (cpd/models/roi_heads/voxel_rcnn_head.py:664-913) in training mode: proposal layer,
                             proposal-target sampling under recorded seeds, canonical targets, the pooling with batch-statistics
                             BatchNorm, RoIHeadTemplate.get_loss and its autograd gradients.
  rcnn_loss.npz              RoIHeadTemplate.get_box_cls_layer_loss + get_box_reg_layer_loss (roi_head_template.py:148-267) called
                             directly on synthetic forward_ret_dicts that reach the edges of the loss (saturated logits, ignored and
                             fractional labels, headings where the flipped ground truth is nearer, boxes apart along one axis,
                             no foreground, nothing valid, a single row).

Only DATA is written. Usage:  python tests/golden/make_golden_rcnn_train.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import AttrDict, _load_roi_stack, setup_reference  # noqa: E402


def _loss_cfg(corner=True, cls_w=1.0, reg_w=1.0, corner_w=1.0, code_weights=(1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)):
    return AttrDict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=corner, GRID_3D_IOU_LOSS=False,
                    LOSS_WEIGHTS=AttrDict(rcnn_cls_weight=cls_w, rcnn_reg_weight=reg_w, rcnn_corner_weight=corner_w,
                                          code_weights=list(code_weights)))


def _target_cfg(per_image):
    return AttrDict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=per_image, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou",
                    CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.02, CLS_BG_THRESH_LO=0.01, HARD_BG_RATIO=0.1, REG_FG_THRESH=0.3)


def _canonical(rois, gt_src):
    """roi_head_template.py:116-146's canonical transformation of (B, N, 8) ground truth into the frames of (B, N, 7) RoIs."""
    b = rois.shape[0]
    gt = gt_src.clone()
    ry = rois[:, :, 6] % (2 * np.pi)
    gt[:, :, 0:3] = gt[:, :, 0:3] - rois[:, :, 0:3]
    gt[:, :, 6] = gt[:, :, 6] - ry
    c, s = torch.cos(-ry.view(-1)), torch.sin(-ry.view(-1))
    x, y = gt.view(-1, gt.shape[-1])[:, 0].clone(), gt.view(-1, gt.shape[-1])[:, 1].clone()
    flat = gt.view(-1, gt.shape[-1])
    flat[:, 0], flat[:, 1] = x * c - y * s, x * s + y * c
    h = gt[:, :, 6] % (2 * np.pi)
    opp = (h > np.pi * 0.5) & (h < np.pi * 1.5)
    h[opp] = (h[opp] + np.pi) % (2 * np.pi)
    h[h > np.pi] = h[h > np.pi] - 2 * np.pi
    gt[:, :, 6] = torch.clamp(h, min=-np.pi / 2, max=np.pi / 2)
    return gt.view(b, -1, gt.shape[-1])


def _loss_case(g, b, n, fg_frac=0.5, labels="mixed", logit_scale=1.0):
    """A synthetic forward_ret_dict: RoIs (some with headings near +-pi/2 and pi), their ground truth (some turned by ~pi, so that
    the flipped box of the corner loss is the nearer one), predictions near the truth with outliers (one axis far off: no overlap)."""
    rows = b * n
    rois = np.zeros((rows, 7), np.float32)
    rois[:, 0:2] = g.uniform(-30, 30, (rows, 2))
    rois[:, 2] = g.uniform(-1, 1, rows)
    rois[:, 3:6] = g.uniform(0.6, 5.0, (rows, 3))
    heads = np.array([np.pi / 2, -np.pi / 2, np.pi, -np.pi, 0.0])
    rois[:, 6] = np.where(g.random(rows) < 0.6, heads[g.integers(0, 5, rows)] + g.normal(0, 0.02, rows), g.uniform(-3.1, 3.1, rows))
    gt = np.zeros((rows, 8), np.float32)
    gt[:, 0:3] = rois[:, 0:3] + g.normal(0, 0.3, (rows, 3))
    gt[:, 3:6] = rois[:, 3:6] * g.uniform(0.8, 1.25, (rows, 3))
    flip = g.random(rows) < 0.35
    gt[:, 6] = rois[:, 6] + g.normal(0, 0.2, rows) + np.where(flip, np.pi, 0.0)
    gt[:, 7] = g.integers(1, 4, rows)
    cls = (g.normal(0, 3, rows) * logit_scale).astype(np.float32)
    sat = g.random(rows) < 0.3
    cls[sat] = g.choice([20.0, -20.0, 40.0, -40.0], int(sat.sum()))
    reg = g.normal(0, 0.3, (rows, 7)).astype(np.float32)
    off = g.random(rows) < 0.15
    reg[off, g.integers(0, 3, int(off.sum()))] = g.choice([-4.0, 4.0], int(off.sum()))         # centre far off along one axis
    mask = (g.random(rows) < fg_frac).astype(np.int64)
    if labels == "mixed":
        lab = np.where(g.random(rows) < 0.4, g.uniform(0, 1, rows), g.integers(0, 2, rows).astype(np.float64))
        lab[g.random(rows) < 0.2] = -1.0
    else:
        lab = np.full(rows, -1.0)
    lab = lab.astype(np.float32)
    t = {"rois": torch.from_numpy(rois).view(b, n, 7), "gt_of_rois_src": torch.from_numpy(gt).view(b, n, 8),
         "reg_valid_mask": torch.from_numpy(mask).view(b, n), "rcnn_cls_labels": torch.from_numpy(lab).view(b, n),
         "rcnn_cls": torch.from_numpy(cls).view(rows, 1), "rcnn_reg": torch.from_numpy(reg)}
    t["gt_of_rois"] = _canonical(t["rois"], t["gt_of_rois_src"])
    return t


def rcnn_loss(R):
    # torch's CPU binary_cross_entropy rejects targets outside [0, 1]; the reference feeds it the -1 (ignore) labels and masks those
    # rows' terms out afterwards (roi_head_template.py:238-240). The ignored rows are handed over as 0 here, which changes nothing the
    # reference keeps: their terms are finite (logs clamped at -100) and multiplied by a zero mask
    bce = torch.nn.functional.binary_cross_entropy
    torch.nn.functional.binary_cross_entropy = lambda inp, tgt, *a, **k: bce(inp, torch.where(tgt >= 0, tgt, torch.zeros_like(tgt)), *a, **k)
    g = np.random.default_rng(5150)
    cases = [
        ("mixed", dict(b=2, n=48), _loss_cfg(code_weights=(1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8))),
        ("weights_no_corner", dict(b=2, n=24), _loss_cfg(corner=False, cls_w=2.0, reg_w=0.5, corner_w=0.7,
                                                          code_weights=(1.0, 0.9, 1.1, 1.0, 1.2, 1.0, 0.5))),
        ("weights_corner", dict(b=1, n=40, fg_frac=0.8), _loss_cfg(cls_w=0.5, reg_w=2.0, corner_w=0.7)),
        ("no_fg", dict(b=2, n=16, fg_frac=0.0), _loss_cfg()),
        ("all_ignored", dict(b=1, n=20, labels="ignored"), _loss_cfg()),
        ("one_row", dict(b=1, n=1, fg_frac=1.0), _loss_cfg()),
    ]
    out = {"names": np.array([c[0] for c in cases])}
    for i, (name, kw, lc) in enumerate(cases):
        t = _loss_case(g, **kw)
        if name == "one_row":
            t["reg_valid_mask"][:] = 1
            t["rcnn_cls_labels"][:] = 0.7
        cfg = AttrDict(TARGET_CONFIG=_target_cfg(kw["n"]), LOSS_CONFIG=lc)
        head = R["rht"].RoIHeadTemplate(num_class=1, num_frames=1, model_cfg=cfg)
        keep = {k: v.clone() for k, v in t.items()}                  # (get_box_reg_layer_loss clamps gt_of_rois' sizes in place)
        t["rcnn_cls"] = t["rcnn_cls"].clone().requires_grad_(True)
        t["rcnn_reg"] = t["rcnn_reg"].clone().requires_grad_(True)
        cls, tb_c = head.get_box_cls_layer_loss(t)
        reg, tb_r = head.get_box_reg_layer_loss(t)
        total = cls + reg
        total.backward()
        p = "c%d_" % i
        for k, v in keep.items():
            out[p + k] = v.numpy()
        out[p + "corner_reg"] = np.int64(lc.CORNER_LOSS_REGULARIZATION)
        out[p + "weights"] = np.array([lc.LOSS_WEIGHTS.rcnn_cls_weight, lc.LOSS_WEIGHTS.rcnn_reg_weight, lc.LOSS_WEIGHTS.rcnn_corner_weight],
                                      np.float64)
        out[p + "code_weights"] = np.array(lc.LOSS_WEIGHTS.code_weights, np.float32)
        out[p + "total"] = np.float64(total.item())
        out[p + "cls"] = np.float64(tb_c["rcnn_loss_cls"])
        out[p + "reg_sl1"] = np.float64(tb_r["rcnn_loss_reg"])
        out[p + "reg_ret"] = np.float64(reg.item())                  # smooth-L1 + corner + bb, what get_box_reg_layer_loss returns
        out[p + "tb_keys"] = np.array(sorted(list(tb_c) + list(tb_r)))
        if "rcnn_loss_corner" in tb_r:
            out[p + "corner"] = np.float64(tb_r["rcnn_loss_corner"])
        out[p + "d_cls"] = t["rcnn_cls"].grad.numpy()
        out[p + "d_reg"] = t["rcnn_reg"].grad.numpy()
        print("rcnn_loss %-18s rows %3d fg %3d total %.6f keys %s" % (name, t["rcnn_reg"].shape[0], int((keep["reg_valid_mask"] > 0).sum()),
                                                                      total.item(), sorted(list(tb_c) + list(tb_r))))
    torch.nn.functional.binary_cross_entropy = bce
    np.savez_compressed(os.path.join(HERE, "rcnn_loss.npz"), **out)


def voxel_rcnn_head_train(R):
    """The proto_head scene recipe of make_golden.py (GRID_SIZE 2, DP_RATIO 0: dropout masks are not reproducible across devices),
    without css_score; the reference's VoxelRCNNHead instead of the prototype head. Own seeds."""
    pool = AttrDict(FEATURES_SOURCE=["x_conv3", "x_conv4"], PRE_MLP=True, GRID_SIZE=2, POOL_LAYERS=AttrDict(
        x_conv3=AttrDict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[0.6, 1.2], NSAMPLE=[8, 8], POOL_METHOD="max_pool"),
        x_conv4=AttrDict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[1.2, 2.4], NSAMPLE=[8, 8], POOL_METHOD="max_pool")))
    cfg = AttrDict(
        CLASS_AGNOSTIC=True, ROI_GRID_POOL=pool, SHARED_FC=[48, 48], CLS_FC=[32, 32], REG_FC=[32, 32], DP_RATIO=0.0,
        TARGET_CONFIG=_target_cfg(24), LOSS_CONFIG=_loss_cfg(code_weights=(1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8)),
        NMS_CONFIG=AttrDict(TRAIN=AttrDict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=400, NMS_POST_MAXSIZE=60, NMS_THRESH=0.8)))
    pcr = np.array([-20.8, -20.8, -2.0, 20.8, 20.8, 4.0], np.float32)
    g = np.random.default_rng(2718)
    torch.manual_seed(2718)
    head = R["vrh"].VoxelRCNNHead(input_channels={"x_conv3": 8, "x_conv4": 12}, model_cfg=cfg, point_cloud_range=pcr,
                                  voxel_size=[0.1, 0.1, 0.15], num_class=1).train()
    with torch.no_grad():
        for mm in head.modules():
            if isinstance(mm, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mm.weight.uniform_(0.6, 1.4); mm.bias.normal_(0, 0.2)
        for stack in (head.cls_layers, head.reg_layers):
            stack[-1].weight.normal_(0, 0.08)
    B, n_gt = 2, 7
    gt = np.zeros((B, n_gt + 2, 8), np.float32)
    sizes = np.array([[4.6, 2.0, 1.7], [0.9, 0.8, 1.7], [1.8, 0.8, 1.7]])
    for b in range(B):
        for i in range(n_gt - b):
            c = g.integers(1, 4)
            gt[b, i] = [g.uniform(-17, 17), g.uniform(-17, 17), g.uniform(-0.3, 0.6), *(sizes[c - 1] * g.uniform(0.9, 1.1, 3)), g.uniform(-3.1, 3.1), c]
    n_prop = 420
    boxes = np.zeros((B, n_prop, 7), np.float32)
    cls = g.normal(-2.0, 1.0, (B, n_prop, 3)).astype(np.float32)
    for b in range(B):
        ng = n_gt - b
        for j in range(n_prop):
            if j < 300:
                src = gt[b, j % ng, :7].copy()
                lvl = [0.03, 0.12, 0.35][(j // ng) % 3]
                src[:3] += g.normal(0, lvl, 3) * [1.0, 1.0, 0.3]
                src[3:6] *= g.uniform(1 - lvl, 1 + lvl, 3)
                src[6] += g.normal(0, lvl)
                boxes[b, j] = src
                cls[b, j, int(gt[b, j % ng, 7]) - 1] = g.normal(1.5, 1.0)
            else:
                boxes[b, j] = [g.uniform(-18, 18), g.uniform(-18, 18), g.uniform(-0.3, 0.6), *g.uniform(0.7, 4.5, 3), g.uniform(-3.1, 3.1)]
    lv = {}
    for name, shp, ch, nvox in (("x_conv3", [11, 104, 104], 8, 1800), ("x_conv4", [5, 52, 52], 12, 700)):
        st = 4 if name == "x_conv3" else 8
        cells = [np.stack([g.integers(0, B, nvox), g.integers(0, shp[0], nvox), g.integers(0, shp[1], nvox), g.integers(0, shp[2], nvox)], 1)]
        for b in range(B):
            for i in range(n_gt - b):
                ctr = ((gt[b, i, :3] - pcr[:3]) / (np.array([0.1, 0.1, 0.15]) * st))
                pts = ctr[None] + g.uniform(-1, 1, (40, 3)) * (gt[b, i, 3:6] / (np.array([0.1, 0.1, 0.15]) * st)) * 0.6
                cz = np.clip(np.floor(pts[:, [2, 1, 0]]).astype(int), 0, np.array(shp) - 1)
                cells.append(np.concatenate([np.full((40, 1), b), cz], 1))
        cl = np.unique(np.concatenate(cells), axis=0).astype(np.int32)
        f = torch.randn(cl.shape[0], ch, generator=torch.Generator().manual_seed(2718 + ch)).requires_grad_(True)
        lv[name] = SimpleNamespace(indices=torch.from_numpy(cl), features=f, spatial_shape=shp, batch_size=B)
    bd = {"batch_size": B, "batch_box_preds": torch.from_numpy(boxes), "batch_cls_preds": torch.from_numpy(cls), "gt_boxes": torch.from_numpy(gt),
          "multi_scale_3d_features": lv, "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}
    sd0 = {"h." + k: v.detach().clone().numpy() for k, v in head.state_dict().items()}
    np.random.seed(31)
    torch.manual_seed(31)
    head(bd)
    t = head.forward_ret_dict
    t["rcnn_cls"].retain_grad()
    t["rcnn_reg"].retain_grad()
    keep = {k: t[k].detach().clone() for k in ("rois", "gt_of_rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "roi_labels",
                                              "reg_valid_mask", "rcnn_cls_labels")}
    loss, tb = head.get_loss()
    loss.backward()
    out = dict(sd0)
    out.update(pcr=pcr, gt=gt, boxes=boxes, cls=cls, seed=np.int64(31), loss=np.float64(loss.item()),
               tb_keys=np.array(sorted(tb)), tb_values=np.array([tb[k] for k in sorted(tb)], np.float64))
    for name in ("x_conv3", "x_conv4"):
        out[name + "_idx"] = lv[name].indices.numpy()
        out[name + "_feat"] = lv[name].features.detach().numpy()
        out[name + "_grad4"] = lv[name].features.grad.numpy()[::4]                  # every 4th row
    for k, v in keep.items():
        out["t_" + k] = v.numpy()
    for k in ("rcnn_cls", "rcnn_reg"):
        out["o_" + k] = t[k].detach().numpy()
        out["d_" + k] = t[k].grad.numpy()
    for k, prm in head.named_parameters():
        if prm.grad is not None and (k.endswith("3.weight") or "mlps_pos" in k or k.startswith("shared_fc_layers.0") or k.endswith("0.0.weight")
                                     or k.startswith("cls_layers.6") or k.startswith("reg_layers.6")):
            out["g." + k] = prm.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "voxel_rcnn_head_train.npz"), **out)
    print("voxel_rcnn_head_train: loss %.6f, %d fg of %d rois, tb %s, %d gradient arrays" % (
        loss.item(), int((keep["reg_valid_mask"] > 0).sum()), keep["reg_valid_mask"].numel(), tb, sum(k.startswith("g.") for k in out)))


def main():
    R = _load_roi_stack(setup_reference())
    rcnn_loss(R)
    voxel_rcnn_head_train(R)


if __name__ == "__main__":
    main()
