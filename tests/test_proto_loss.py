"""CPU: the torch restatement of VoxelRCNNProtoHead's loss (roi_head_train.proto_head_loss_torch) against the reference's own
VoxelRCNNProtoHead.get_loss on the edge cases of tests/golden/proto_loss.npz (make_golden_proto_loss.py): the total, the pieces the
reference's methods return one by one, and the autograd gradients with respect to both branches' rcnn_cls / rcnn_reg and the detection
branch's shared features; and the head's `fused_loss` switch."""
import numpy as np
import pytest
import torch

NAMES = ["mixed", "weights", "weights_corner", "no_fg", "css_off_on_fg", "css_all_zero", "equal_branches", "one_row", "degenerate_features",
         "ramp_1", "ramp_5000", "ramp_6000"]
CASES = range(len(NAMES))
INPUTS = ("cls0", "reg0", "feat0", "cls1", "reg1", "feat1", "rois", "gt_of_rois", "gt_of_rois_src", "reg_valid_mask", "rcnn_cls_labels", "css")
LEAVES = ("cls0", "reg0", "feat0", "cls1", "reg1")


def case(g, i, device="cpu"):
    """-> (the twelve row inputs of proto_head_loss_torch / proto_loss_fused in order, the keyword arguments)."""
    from cpd_amd.roi_head_train import proto_ramp_weight
    p = "c%d_" % i
    w = g[p + "weights"]
    args = [torch.from_numpy(g[p + k]).to(device) for k in INPUTS]
    return args, dict(code_weights=g[p + "code_weights"].tolist(), cls_weight=float(w[0]), reg_weight=float(w[1]), corner_weight=float(w[2]),
                      proto_weight=float(w[3]), ramp_weight=proto_ramp_weight(int(g[p + "iter"])), corner_regularization=bool(g[p + "corner_reg"]))


def restated(args, kw, grad=True):
    from cpd_amd.roi_head_train import proto_head_loss_torch
    leaves = [a.clone().requires_grad_(grad) for a in args[:5]]
    total, terms = proto_head_loss_torch(*leaves, *args[5:], **kw)
    if grad:
        total.backward()
    return leaves, total, terms


def rows_close(got, want, rtol, atol=0.0):
    """Every row of `got` within rtol of that row's own largest |want| (+ atol); -> the worst row's error over its bound."""
    got, want = np.asarray(got, np.float64).reshape(want.shape[0], -1), np.asarray(want, np.float64).reshape(want.shape[0], -1)
    if want.size == 0:
        return 0.0
    err, bound = np.abs(got - want).max(axis=1), rtol * np.abs(want).max(axis=1) + atol
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


def _rel(got, want):
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-12)


def test_fixture_covers_the_edges(golden):
    g = golden("proto_loss")
    assert list(g["names"]) == NAMES
    count = {}
    for i, name in enumerate(NAMES):
        p = "c%d_" % i
        mask, css, lab = g[p + "reg_valid_mask"].ravel(), g[p + "css"].ravel(), g[p + "rcnn_cls_labels"].ravel()
        assert (lab >= 0).all() and (lab <= 1).all()
        fgp = mask > 0
        assert (g[p + "gt_of_rois"].reshape(-1, 8)[fgp, 3:6] > 1e-5).all() and (g[p + "rois"].reshape(-1, 7)[fgp, 3:6] > 1e-5).all()
        count[name] = (mask.size, int(fgp.sum()), int((mask * css > 0).sum()), float(css.sum()))
    rows, fp, fc, _ = count["mixed"]
    assert rows == 96 and g["c0_feat0"].shape == (96, 48) and 0 < fc < fp
    css = g["c0_css"].ravel()
    assert (css == 0).any() and ((css == 0) | ((css >= 0.2) & (css <= 1))).all()
    lab = g["c0_rcnn_cls_labels"].ravel()
    assert ((lab > 0) & (lab < 1)).any() and (lab == 0).any() and (lab == 1).any()
    assert set(np.abs(np.concatenate([g["c0_cls0"], g["c0_cls1"]])).ravel().tolist()) >= {20.0, 40.0}
    assert (np.abs(g["c0_reg0"][:, 0:3]) == 4.0).any()                                  # a centre axis far off
    w = g["c1_weights"]
    assert not g["c1_corner_reg"] and (w != 1).all() and (g["c1_code_weights"] != 1).any()
    assert count["no_fg"][1] == 0
    assert count["css_off_on_fg"][1] > 0 and count["css_off_on_fg"][2] == 0 and count["css_off_on_fg"][3] > 0
    assert count["css_all_zero"][3] == 0 and count["css_all_zero"][1] > 0
    i = NAMES.index("equal_branches")
    assert np.array_equal(g["c%d_reg0" % i], g["c%d_reg1" % i]) and count["equal_branches"][1] > 0
    assert count["one_row"][:3] == (1, 1, 1)
    i = NAMES.index("degenerate_features")
    n0, n1 = np.linalg.norm(g["c%d_feat0" % i], axis=1), np.linalg.norm(g["c%d_feat1" % i], axis=1)
    assert (n0 == 0).sum() == 2 and (n1 == 0).sum() == 2 and ((n0 > 0) & (n0 < 1e-8)).sum() == 2 and ((n1 > 0) & (n1 < 1e-8)).sum() == 2
    assert (g["c%d_css" % i].ravel()[:6] > 0).all()
    assert [int(g["c%d_iter" % NAMES.index(n)]) for n in NAMES[-3:]] == [1, 5000, 6000]
    assert [int(g["c%d_iter_after" % NAMES.index(n)]) for n in NAMES[-3:]] == [2, 5001, 5001]


@pytest.mark.parametrize("i", CASES)
def test_restatement_matches_reference_total_and_pieces(golden, i):
    g = golden("proto_loss")
    p = "c%d_" % i
    _, total, terms = restated(*case(g, i), grad=False)

    def close(got, key):
        want = float(g[p + key])
        assert _rel(got, want) <= 1e-6 or float(got) == want == 0, (key, float(got), want)
    close(total, "total")
    close(total, "tb_rcnn_loss")
    for j in (0, 1):
        close(terms["cls%d" % j], "loss_cls%d" % j)
        close(terms["reg%d" % j], "loss_reg%d" % j)
        close(terms["reg%d" % j] + terms["corner%d" % j], "loss_reg_ret%d" % j)
        if p + "loss_corner%d" % j in g.files:
            close(terms["corner%d" % j], "loss_corner%d" % j)
        else:
            assert float(terms["corner%d" % j]) == 0
    close(terms["b0"] + terms["b1"] + terms["feat"], "loss_proto")
    mask, css = g[p + "reg_valid_mask"].ravel(), g[p + "css"].ravel()
    assert (terms["Fc"], terms["Fp"]) == (int((mask * css > 0).sum()), int((mask > 0).sum()))
    assert float(terms["total"]) == float(total)


@pytest.mark.parametrize("i", CASES)
def test_restatement_gradients_match_reference(golden, i):
    g = golden("proto_loss")
    p = "c%d_" % i
    leaves, _, _ = restated(*case(g, i))
    for leaf, key in zip(leaves, LEAVES):
        want = g[p + "d_" + key]
        assert leaf.grad.shape == want.shape
        if key == "feat0":                        # row by row: a degenerate row's gradient (~1e7) would hide every other row's
            assert rows_close(leaf.grad.numpy(), want, 1e-6) <= 1.0, key
        else:
            err = np.abs(leaf.grad.numpy() - want).max()
            assert err <= 1e-6 * max(np.abs(want).max(), 1.0), (key, err)


def test_ramp_weight_follows_the_reference():
    from cpd_amd.roi_head_train import proto_ramp_weight
    assert proto_ramp_weight(1) == (1 / 5000) * (0.2 - 0.00001) + 0.00001
    assert proto_ramp_weight(5000) == proto_ramp_weight(6000) == 1.0 * (0.2 - 0.00001) + 0.00001


def _pool_cfg():
    return dict(FEATURES_SOURCE=["x_conv3"], PRE_MLP=True, GRID_SIZE=2, POOL_LAYERS=dict(
        x_conv3=dict(MLPS=[[8, 8]], QUERY_RANGES=[[1, 1, 1]], POOL_RADIUS=[0.6], NSAMPLE=[4], POOL_METHOD="max_pool")))


def _head_cfg(**extra):
    return dict(CLASS_AGNOSTIC=True, ROI_GRID_POOL=_pool_cfg(), SHARED_FC=[16], CLS_FC=[16], REG_FC=[16], DP_RATIO=0.0,
                TARGET_CONFIG=dict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=8, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou",
                                   CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.02, CLS_BG_THRESH_LO=0.01, HARD_BG_RATIO=0.1, REG_FG_THRESH=0.3),
                LOSS_CONFIG=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True, GRID_3D_IOU_LOSS=False,
                                 LOSS_WEIGHTS=dict(rcnn_proto_weight=1.0, rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0,
                                                   code_weights=[1.0] * 7)),
                NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=16, NMS_THRESH=0.8)), **extra)


def test_set_fused_loss_flips_the_prototype_heads_only():
    from cpd_amd import roi_pool
    from cpd_amd.roi_head_train import VoxelRCNNProtoHead, set_fused_loss
    kw = dict(input_channels={"x_conv3": 4}, point_cloud_range=[-20.8, -20.8, -2.0, 20.8, 20.8, 4.0], voxel_size=[0.1, 0.1, 0.15], num_class=1)
    proto = VoxelRCNNProtoHead(model_cfg=_head_cfg(ROI_GRID_POOL_PROTO=_pool_cfg()), **kw)
    anchor = roi_pool.VoxelRCNNHead(model_cfg=_head_cfg(), **kw)
    assert proto.fused_loss is False and proto.last_losses is None
    assert set_fused_loss(torch.nn.ModuleList([proto, anchor])) == 1 and proto.fused_loss is True
    assert set_fused_loss(anchor) == 0 and not hasattr(anchor, "fused_loss")
    assert set_fused_loss(proto, on=False) == 1 and proto.fused_loss is False


def test_uncovered_loss_options_still_raise():
    from cpd_amd.roi_head_train import VoxelRCNNProtoHead
    for key, value in (("CLS_LOSS", "CrossEntropy"), ("REG_LOSS", "l1")):
        cfg = _head_cfg(ROI_GRID_POOL_PROTO=_pool_cfg())
        cfg["LOSS_CONFIG"][key] = value
        head = VoxelRCNNProtoHead(input_channels={"x_conv3": 4}, model_cfg=cfg, point_cloud_range=[-20.8, -20.8, -2.0, 20.8, 20.8, 4.0],
                                  voxel_size=[0.1, 0.1, 0.15], num_class=1)
        head.fused_loss = True
        head.forward_ret_dict = {"targets_dict0": {}, "targets_dict1": {}}
        with pytest.raises(NotImplementedError):
            head.get_loss()
        assert head.iter == 1


def test_bad_arguments_are_refused_before_any_launch():
    from cpd_amd._lib import farr, lib
    rows = farr([0.0] * 16)                       # never read: every call below fails its argument check
    call = lambda feat_dim, ld_gt, n, losses, first=rows: lib().cpd_rcnn_proto_loss(
        first, rows, rows, rows, rows, rows, feat_dim, rows, rows, ld_gt, rows, 7, rows, rows, rows, n, farr([1.0] * 7), 1.0, 1.0, 1.0, 1.0, 0.2,
        1, rows, rows, rows, rows, rows, losses, None)
    assert call(0, 7, 1, rows) == -1 and call(1, 6, 1, rows) == -1 and call(1, 7, 1, None) == -1 and call(1, 7, -1, rows) == -1
    assert call(1, 7, 1, rows, first=None) == -1
