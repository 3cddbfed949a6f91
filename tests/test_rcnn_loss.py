"""CPU: the torch restatement of the anchor-head VoxelRCNN's RoI loss (roi_head_train.rcnn_head_loss_torch) against the
reference's own RoIHeadTemplate.get_box_cls_layer_loss + get_box_reg_layer_loss on the edge cases of tests/golden/rcnn_loss.npz
(make_golden_rcnn_train.py): loss terms, tb_dict keys and the autograd gradients with respect to rcnn_cls / rcnn_reg."""
import numpy as np
import pytest
import torch

CASES = range(6)


def restated(g, i, grad=True):
    from cpd_amd.roi_head_train import rcnn_head_loss_torch
    p = "c%d_" % i
    cls = torch.from_numpy(g[p + "rcnn_cls"]).requires_grad_(grad)
    reg = torch.from_numpy(g[p + "rcnn_reg"]).requires_grad_(grad)
    w = g[p + "weights"]
    total, terms = rcnn_head_loss_torch(cls, reg, torch.from_numpy(g[p + "rois"]), torch.from_numpy(g[p + "gt_of_rois"]),
                                        torch.from_numpy(g[p + "gt_of_rois_src"]), torch.from_numpy(g[p + "reg_valid_mask"]),
                                        torch.from_numpy(g[p + "rcnn_cls_labels"]), g[p + "code_weights"].tolist(), float(w[0]), float(w[1]),
                                        float(w[2]), bool(g[p + "corner_reg"]))
    return cls, reg, total, terms


def _rel(got, want):
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-12)


def test_fixture_covers_the_edges(golden):
    g = golden("rcnn_loss")
    names = list(g["names"])
    assert names == ["mixed", "weights_no_corner", "weights_corner", "no_fg", "all_ignored", "one_row"]
    for i in CASES:
        p = "c%d_" % i
        fg = int((g[p + "reg_valid_mask"] > 0).sum())
        lab = g[p + "rcnn_cls_labels"]
        if names[i] == "no_fg":
            assert fg == 0
        if names[i] == "all_ignored":
            assert (lab < 0).all() and fg > 0
        if names[i] == "one_row":
            assert g[p + "rcnn_reg"].shape == (1, 7) and fg == 1
    mixed = g["c0_rcnn_cls_labels"]
    assert ((mixed > 0) & (mixed < 1)).any() and (mixed == 0).any() and (mixed == 1).any() and (mixed < 0).any()
    assert set(np.abs(g["c0_rcnn_cls"]).ravel().tolist()) >= {20.0, 40.0}


@pytest.mark.parametrize("i", CASES)
def test_restatement_matches_reference_terms_and_keys(golden, i):
    g = golden("rcnn_loss")
    p = "c%d_" % i
    _, _, total, terms = restated(g, i, grad=False)
    assert _rel(total, g[p + "total"]) <= 1e-6, (float(total), float(g[p + "total"]))
    assert _rel(terms["rcnn_loss_cls"], g[p + "cls"]) <= 1e-6
    assert _rel(terms["rcnn_loss_reg"], g[p + "reg_sl1"]) <= 1e-6 or abs(float(g[p + "reg_sl1"])) == float(terms["rcnn_loss_reg"]) == 0
    reg_ret = float(terms["rcnn_loss_reg"]) + float(terms.get("rcnn_loss_corner", 0.0)) + float(terms["rcnn_loss_bb"])
    assert _rel(reg_ret, g[p + "reg_ret"]) <= 1e-6
    keys = sorted(k for k in terms if k.startswith("rcnn_loss_") and k != "rcnn_loss_bb")
    assert keys == sorted(g[p + "tb_keys"].tolist())
    if p + "corner" in g.files:
        assert _rel(terms["rcnn_loss_corner"], g[p + "corner"]) <= 1e-6
    else:
        assert "rcnn_loss_corner" not in terms


@pytest.mark.parametrize("i", CASES)
def test_restatement_gradients_match_reference(golden, i):
    g = golden("rcnn_loss")
    p = "c%d_" % i
    cls, reg, total, _ = restated(g, i)
    total.backward()
    for got, key in ((cls.grad, "d_cls"), (reg.grad, "d_reg")):
        want = g[p + key]
        err = np.abs(got.numpy() - want).max()
        assert err <= 1e-6 * max(np.abs(want).max(), 1.0), (key, err)
