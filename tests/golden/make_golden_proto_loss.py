#!/usr/bin/env python3
"""Golden vectors of VoxelRCNNProtoHead's loss (run in the build container only, like make_golden.py, whose loaders it imports): the
REFERENCE's own class, loaded by file path, on CPU.

  proto_loss.npz  VoxelRCNNProtoHead.get_loss (cpd/models/roi_heads/voxel_rcnn_head.py:388-579) on synthetic targets_dict0 /
                  targets_dict1 set by hand, with `head.iter` set by hand: the total, its autograd gradients with respect to both
                  branches' rcnn_cls / rcnn_reg and the detection branch's shared_features, and the pieces -- get_box_cls_layer_loss,
                  get_box_reg_layer_loss and proto_loss called one by one on fresh clones at the same iter. The cases reach the edges
                  of the loss: zero prototype confidences on foreground rows, no foreground, all confidences zero, equal branches
                  (every min / max of bb_loss ties), a single row, zero and near-zero feature vectors, the ramp's ends.
                  Labels lie in [0, 1] and foreground rows have sizes above 1e-5, where the reference's methods are defined.

Only DATA is written. Usage:  python tests/golden/make_golden_proto_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import AttrDict, _load_roi_stack, setup_reference  # noqa: E402
from make_golden_rcnn_train import _loss_case, _target_cfg  # noqa: E402

TARGET_KEYS = ("rois", "gt_of_rois", "gt_of_rois_src", "reg_valid_mask", "rcnn_cls_labels")


def _head(R, per_image, lw):
    pool = lambda: AttrDict(FEATURES_SOURCE=["x_conv3"], PRE_MLP=True, GRID_SIZE=2, POOL_LAYERS=AttrDict(
        x_conv3=AttrDict(MLPS=[[8, 8]], QUERY_RANGES=[[1, 1, 1]], POOL_RADIUS=[0.6], NSAMPLE=[4], POOL_METHOD="max_pool")))
    cfg = AttrDict(CLASS_AGNOSTIC=True, ROI_GRID_POOL=pool(), ROI_GRID_POOL_PROTO=pool(), SHARED_FC=[16], CLS_FC=[16], REG_FC=[16], DP_RATIO=0.0,
                   TARGET_CONFIG=_target_cfg(per_image),
                   LOSS_CONFIG=AttrDict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=lw["corner"],
                                        GRID_3D_IOU_LOSS=False,
                                        LOSS_WEIGHTS=AttrDict(rcnn_proto_weight=lw["proto"], rcnn_cls_weight=lw["cls"], rcnn_reg_weight=lw["reg"],
                                                              rcnn_corner_weight=lw["corner_w"], rcnn_iou3d_weight=1.0,
                                                              code_weights=list(lw["code"]))))
    return R["vrh"].VoxelRCNNProtoHead(input_channels={"x_conv3": 4}, model_cfg=cfg, point_cloud_range=np.array([-20.8, -20.8, -2.0, 20.8, 20.8, 4.0], np.float32),
                                       voxel_size=[0.1, 0.1, 0.15], num_class=1).train()


def _weights(corner=True, cls=1.0, reg=1.0, corner_w=1.0, proto=1.0, code=(1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8)):
    return dict(corner=corner, cls=cls, reg=reg, corner_w=corner_w, proto=proto, code=code)


def _case(g, b, n, width, fg_frac=0.5):
    """make_golden_rcnn_train's synthetic rows (RoIs with headings near +-pi/2 and pi, source gts turned by pi, saturated logits, one
    centre axis far off) with labels in [0, 1], a prototype branch, shared features and prototype confidences in {0} + [0.2, 1]."""
    t = _loss_case(g, b=b, n=n, fg_frac=fg_frac)
    rows = b * n
    lab = t["rcnn_cls_labels"].view(-1)
    ignored = lab < 0
    lab[ignored] = torch.from_numpy(g.choice([0.0, 1.0, 0.35], int(ignored.sum())).astype(np.float32))
    t1 = _loss_case(g, b=b, n=n, fg_frac=fg_frac)                                       # the prototype branch's logits and residuals
    css = np.where(g.random(rows) < 0.25, 0.0, g.uniform(0.2, 1.0, rows)).astype(np.float32)
    out = {k: t[k] for k in TARGET_KEYS}
    out["css"] = torch.from_numpy(css).view(b, n)
    out["cls0"], out["reg0"], out["cls1"], out["reg1"] = t["rcnn_cls"], t["rcnn_reg"], t1["rcnn_cls"], t1["rcnn_reg"]
    out["feat0"] = torch.from_numpy(np.maximum(g.normal(0.2, 1.0, (rows, width)), 0).astype(np.float32))   # post-ReLU features
    out["feat1"] = torch.from_numpy(np.maximum(g.normal(0.2, 1.0, (rows, width)), 0).astype(np.float32))
    return out


def _dicts(c, grad):
    """targets_dict0 / targets_dict1 as VoxelRCNNProtoHead.forward leaves them: clones of one target dict, each with its branch."""
    leaves = {k: c[k].clone().requires_grad_(grad) for k in ("cls0", "reg0", "feat0", "cls1", "reg1", "feat1")}
    ts = []
    for j in (0, 1):
        t = {k: c[k].clone() for k in TARGET_KEYS}
        t["additional_data"] = {"css_score": c["css"].clone()}
        t.update(rcnn_cls=leaves["cls%d" % j], rcnn_reg=leaves["reg%d" % j], shared_features=leaves["feat%d" % j])
        ts.append(t)
    return leaves, ts


def main():
    R = _load_roi_stack(setup_reference())
    g = np.random.default_rng(388)
    cases = []

    def add(name, c, lw=None, it=1):
        cases.append((name, c, lw or _weights(), it))
    add("mixed", _case(g, 2, 48, 48), it=1200)
    add("weights", _case(g, 2, 12, 16), _weights(corner=False, cls=2.0, reg=0.5, corner_w=0.7, proto=0.6, code=(1.0, 0.9, 1.1, 1.0, 1.2, 1.0, 0.5)), it=2500)
    add("weights_corner", _case(g, 1, 16, 8, fg_frac=0.8), _weights(cls=0.5, reg=2.0, corner_w=0.7, proto=1.5), it=4000)
    add("no_fg", _case(g, 2, 8, 8, fg_frac=0.0), it=3000)
    c = _case(g, 2, 8, 8)
    c["css"][c["reg_valid_mask"] > 0] = 0.0
    add("css_off_on_fg", c, it=3000)
    c = _case(g, 1, 12, 8)
    c["css"][:] = 0.0
    add("css_all_zero", c, it=3000)
    c = _case(g, 1, 16, 8, fg_frac=0.7)
    c["reg1"] = c["reg0"].clone()
    add("equal_branches", c, it=5000)
    c = _case(g, 1, 1, 16, fg_frac=1.0)
    c["reg_valid_mask"][:] = 1
    c["rcnn_cls_labels"][:] = 0.7
    c["css"][:] = 0.6
    add("one_row", c, it=700)
    c = _case(g, 1, 16, 16)
    c["css"][0, :8] = torch.from_numpy(g.uniform(0.2, 1.0, 8).astype(np.float32))        # the degenerate rows all carry weight
    c["feat0"][0] = 0.0
    c["feat1"][1] = 0.0
    c["feat0"][2] = torch.from_numpy(np.abs(g.normal(0, 1e-10, 16)).astype(np.float32))   # norm below the 1e-8 clamp
    c["feat1"][3] = torch.from_numpy(np.abs(g.normal(0, 1e-10, 16)).astype(np.float32))
    c["feat0"][4] = 0.0
    c["feat1"][4] = 0.0
    c["feat0"][5] = torch.from_numpy(np.abs(g.normal(0, 1e-10, 16)).astype(np.float32))
    c["feat1"][5] = torch.from_numpy(np.abs(g.normal(0, 1e-10, 16)).astype(np.float32))
    add("degenerate_features", c, it=5000)
    c = _case(g, 1, 12, 8)
    for it in (1, 5000, 6000):
        add("ramp_%d" % it, c, it=it)

    out = {"names": np.array([c[0] for c in cases])}
    for i, (name, c, lw, it) in enumerate(cases):
        per_image = c["rois"].shape[1]
        head = _head(R, per_image, lw)
        leaves, (t0, t1) = _dicts(c, True)
        head.forward_ret_dict = {"targets_dict0": t0, "targets_dict1": t1}
        head.iter = it
        total, tb = head.get_loss()
        total.backward()
        assert sorted(tb) == ["rcnn_loss"], tb
        p = "c%d_" % i
        for k, v in c.items():
            out[p + k] = v.numpy()
        out[p + "corner_reg"] = np.int64(lw["corner"])
        out[p + "weights"] = np.array([lw["cls"], lw["reg"], lw["corner_w"], lw["proto"]], np.float64)
        out[p + "code_weights"] = np.array(lw["code"], np.float32)
        out[p + "iter"], out[p + "iter_after"] = np.int64(it), np.int64(head.iter)
        out[p + "total"] = np.float64(total.item())
        out[p + "tb_rcnn_loss"] = np.float64(tb["rcnn_loss"])
        for k in ("cls0", "reg0", "feat0", "cls1", "reg1"):
            out[p + "d_" + k] = leaves[k].grad.numpy()
        assert leaves["feat1"].grad is None
        # the pieces, one by one on fresh clones at the same iter
        _, (u0, u1) = _dicts(c, False)
        for j, u in enumerate((u0, u1)):
            cls, _ = head.get_box_cls_layer_loss(u)
            reg, tb_r = head.get_box_reg_layer_loss(u)
            out[p + "loss_cls%d" % j] = np.float64(cls.item())
            out[p + "loss_reg%d" % j] = np.float64(tb_r["rcnn_loss_reg"])
            out[p + "loss_reg_ret%d" % j] = np.float64(reg.item())                   # smooth-L1 + corner, what get_box_reg_layer_loss returns
            if "rcnn_loss_corner" in tb_r:
                out[p + "loss_corner%d" % j] = np.float64(tb_r["rcnn_loss_corner"])
        head.iter = it
        proto = head.proto_loss(u0, u1)                                          # b0 + b1 + feat (after get_box_reg_layer_loss's clamp)
        out[p + "loss_proto"] = np.float64(float(proto))
        mask, css = c["reg_valid_mask"].view(-1), c["css"].view(-1)
        print("proto_loss %-20s rows %3d width %2d Fp %3d Fc %3d Sv %7.3f iter %4d -> %4d total %.6f proto %.6f" % (
            name, mask.numel(), c["feat0"].shape[1], int((mask > 0).sum()), int((mask * css > 0).sum()), float(css.sum()), it, head.iter,
            total.item(), float(proto)))
    np.savez_compressed(os.path.join(HERE, "proto_loss.npz"), **out)


if __name__ == "__main__":
    main()
