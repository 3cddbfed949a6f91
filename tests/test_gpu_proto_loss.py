"""GPU: the fused loss-and-gradient kernel of the prototype RoI head, `cpd_rcnn_proto_loss` -- against its torch restatement
(roi_head_train.proto_head_loss_torch, itself pinned on the reference in test_proto_loss.py) on the reference's edge cases and on random
rows at the kernel's lane / wave strides, against the reference's totals, and through VoxelRCNNProtoHead.fused_loss: the head's training
step against the reference's (tests/golden/proto_head.npz) and the two-stage detector's training forward against the unfused one."""
import types

import numpy as np
import pytest
import torch

from test_proto_loss import CASES, NAMES, case, restated, rows_close

pytestmark = pytest.mark.gpu

OUTPUTS = ("d_cls0", "d_reg0", "d_feat0", "d_cls1", "d_reg1")


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _check_against_restatement(args, kw, what):
    """The twelve losses and the five gradients at 1e-5 |want| + 1e-7 (cpd_rcnn_loss's tolerance; the gradients against the tensor's
    largest entry, d_feat0 row by row -- a degenerate row's gradient is ~1e7); a second call is bitwise equal. -> the kernel's losses."""
    from cpd_amd.roi_head_train import PROTO_TERMS, proto_loss_fused
    leaves, _, terms = restated(args, kw)
    out = proto_loss_fused(*args, **kw)
    got = out[0].cpu().numpy().astype(np.float64)
    assert got.shape == (12,)
    for k, name in enumerate(PROTO_TERMS):
        want = float(terms[name].detach()) if torch.is_tensor(terms[name]) else float(terms[name])
        print(what, name, got[k], want)
        assert abs(got[k] - want) <= 1e-5 * abs(want) + 1e-7, (what, name, got[k], want)
    for g, leaf, name in zip(out[1:], leaves, OUTPUTS):
        ref = leaf.grad
        assert g.shape == ref.shape and g.dtype == torch.float32, (what, name)
        if name == "d_feat0":
            worst = rows_close(g.cpu().numpy(), ref.cpu().numpy(), 1e-5, 1e-7)
            print(what, name, "worst row error / bound", worst)
            assert worst <= 1.0, (what, name, worst)
        else:
            err = float((g - ref).abs().max()) if ref.numel() else 0.0
            print(what, name, err, float(ref.abs().max()) if ref.numel() else 0.0)
            assert err <= 1e-5 * float(ref.abs().max()) + 1e-7, (what, name, err, float(ref.abs().max()))
    again = proto_loss_fused(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), what
    return got


@pytest.mark.parametrize("i", CASES)
def test_fused_proto_loss_matches_restatement_and_reference_total(golden, hip, i):
    g = golden("proto_loss")
    got = _check_against_restatement(*case(g, i, "cuda"), NAMES[i])
    want = float(g["c%d_total" % i])
    assert abs(got[0] - want) <= 2e-5 * abs(want), (NAMES[i], got[0], want)
    if NAMES[i] in ("no_fg", "css_off_on_fg", "css_all_zero"):
        assert got[3] == got[6] == got[7] == got[8] == 0.0                               # no corner term; b0 / b1 zero sums
    if NAMES[i] == "css_all_zero":
        assert not got[:11].any() and got[11] > 0


def _random_case(n, width, seed):
    """n rows like tests/test_gpu_rcnn_head_train.py's, both branches: headings across the circle, saturated logits, fractional / 0 / 1
    and ignored (-1) labels, about half foreground, prototype confidences in {0} + [0.2, 1], post-ReLU features."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen)
    nrm = lambda *s: torch.randn(*s, generator=gen)
    rois = torch.cat([(r(n, 2) - 0.5) * 60, r(n, 1) - 0.5, 0.6 + 4 * r(n, 3), (r(n, 1) - 0.5) * 6.4], 1)
    edge = r(n) < 0.3
    rois[edge, 6] = torch.tensor([np.pi / 2, -np.pi / 2, np.pi, -np.pi])[torch.randint(0, 4, (int(edge.sum()),), generator=gen)]
    gt_ct = torch.cat([nrm(n, 3) * 0.4, rois[:, 3:6] * (0.8 + 0.45 * r(n, 3)), (r(n, 1) - 0.5) * 3.0, torch.ones(n, 1)], 1)
    src = torch.cat([rois[:, 0:3] + nrm(n, 3) * 0.4, gt_ct[:, 3:6], rois[:, 6:7] + nrm(n, 1) * 0.2 + np.pi * (r(n, 1) < 0.3).float(),
                     torch.ones(n, 1)], 1)
    branches = []
    for _ in (0, 1):
        cls = nrm(n, 1) * 4
        sat = r(n) < 0.1
        cls[sat, 0] = torch.tensor([20.0, -20.0, 40.0, -40.0])[torch.randint(0, 4, (int(sat.sum()),), generator=gen)]
        branches.append((cls, nrm(n, 7) * 0.3, torch.relu(nrm(n, width) + 0.2)))
    lab = torch.where(r(n) < 0.4, r(n), (r(n) < 0.5).float())
    lab[r(n) < 0.15] = -1.0
    mask = (r(n) < 0.5).long()
    css = torch.where(r(n) < 0.25, torch.zeros(n), 0.2 + 0.8 * r(n))
    (c0, r0, f0), (c1, r1, f1) = branches
    args = [c0, r0, f0, c1, r1, f1, rois.view(1, n, 7), gt_ct.view(1, n, 8), src.view(1, n, 8), mask.view(1, n), lab.view(1, n), css.view(1, n)]
    return [a.cuda() for a in args], dict(code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8], cls_weight=1.0, reg_weight=1.0, corner_weight=1.0,
                                          proto_weight=0.8, ramp_weight=0.13, corner_regularization=True)


@pytest.mark.parametrize("n,width", [(1, 1), (63, 48), (255, 31), (256, 64), (257, 257), (520, 256)])
def test_fused_proto_loss_matches_restatement_on_random_rows(hip, n, width):
    args, kw = _random_case(n, width, seed=1000 + n)
    if n > 1:
        assert bool((args[10] < 0).any()) and bool((args[9] > 0).any())
    _check_against_restatement(args, kw, "n=%d width=%d" % (n, width))


def test_fused_proto_loss_without_rows_writes_zero_losses(hip):
    from cpd_amd.roi_head_train import proto_loss_fused
    z = lambda *s: torch.zeros(*s, device="cuda")
    out = proto_loss_fused(z(0, 1), z(0, 7), z(0, 48), z(0, 1), z(0, 7), z(0, 48), z(1, 0, 7), z(1, 0, 8), z(1, 0, 8), z(1, 0), z(1, 0), z(1, 0),
                           [1.0] * 7)
    assert out[0].shape == (12,) and float(out[0].abs().sum()) == 0.0
    assert [tuple(t.shape) for t in out[1:]] == [(0, 1), (0, 7), (0, 48), (0, 1), (0, 7)]


# ---------------------------------------------------------------------------------------------------------------- the head
def test_proto_head_training_step_with_fused_loss_matches_reference(golden, hip):
    """tests/test_gpu_roi_train.py::test_proto_head_training_step_matches_reference's step with fused_loss on, at its tolerances."""
    from cpd_amd import ops
    from cpd_amd.roi_head_train import VoxelRCNNProtoHead, set_fused_loss
    from test_gpu_roi_train import _cfg, _close
    g = golden("proto_head")
    head = VoxelRCNNProtoHead(input_channels={"x_conv3": 8, "x_conv4": 12}, model_cfg=_cfg(), point_cloud_range=g["pcr"].tolist(),
                              voxel_size=[0.1, 0.1, 0.15], num_class=1)
    head.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("h.")}, strict=True)
    head = head.cuda().train()
    assert set_fused_loss(head) == 1
    lv, lv_mm = {}, {}
    for name, shp in (("x_conv3", [11, 104, 104]), ("x_conv4", [5, 52, 52])):
        idx = torch.from_numpy(g[name + "_idx"]).cuda()
        for d, key in ((lv, "_feat"), (lv_mm, "_feat_mm")):
            f = torch.from_numpy(g[name + key]).cuda().requires_grad_(True)
            d[name] = types.SimpleNamespace(indices=idx, features=f, spatial_shape=shp, batch_size=2)
    bd = {"batch_size": 2, "batch_box_preds": torch.from_numpy(g["boxes"]).cuda(), "batch_cls_preds": torch.from_numpy(g["cls"]).cuda(),
          "gt_boxes": torch.from_numpy(g["gt"]).cuda(), "css_score": torch.from_numpy(g["css"]).cuda(), "multi_scale_3d_features": lv,
          "multi_scale_3d_features_mm": lv_mm, "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    head(bd)
    with ops.launch_log() as log:
        loss, tb = head.get_loss()
    assert log.counts == {"rcnn_proto_loss_kernel": 1}, log.counts
    assert head.iter == 2
    assert sorted(tb) == ["rcnn_loss"]
    assert abs(loss.item() - float(g["loss"])) <= 2e-4 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))
    assert abs(tb["rcnn_loss"] - float(g["rcnn_loss"])) <= 2e-4 * abs(float(g["rcnn_loss"]))
    assert head.last_losses.shape == (12,) and float(head.last_losses[0]) == loss.item()
    loss.backward()
    params = dict(head.named_parameters())
    n = 0
    for k in g.files:
        if k.startswith("g."):
            _close(params[k[2:]].grad.cpu().numpy(), g[k], "grad " + k[2:], rtol=1e-3, floor=1e-6)
            n += 1
    assert n >= 30
    for name in ("x_conv3", "x_conv4"):
        _close(lv[name].features.grad.cpu().numpy()[::4], g[name + "_grad4"], "d loss / d " + name, rtol=1e-3, floor=1e-7)
        _close(lv_mm[name].features.grad.cpu().numpy()[::4], g[name + "_grad4_mm"], "d loss / d mm " + name, rtol=1e-3, floor=1e-7)


# ---------------------------------------------------------------------------------------------------------------- the detector
def test_two_stage_detector_trains_with_the_fused_loss(hip):
    """tests/test_gpu_two_stage.py's reduced voxel_rcnn_cproto_center detector in training mode (both encoders, CenterHead proposals,
    prototype confidences): the same step on the same seeds with the loss unfused and fused."""
    from cpd_amd import ops
    from cpd_amd.roi_head_train import set_fused_loss
    from test_gpu_two_stage import _clouds, _model
    net = _model().train()
    clouds = _clouds()[:2]
    vox = ops.Voxelizer(net.voxel_size, net.point_cloud_range, 5, 5, 1000000)
    _, coords, _, feats, nvox = vox.batch(clouds)
    n = int(nvox[len(clouds)])

    def batch(gt):
        f, c = feats[:n].clone(), coords[:n].float()
        return {"voxel_features": f, "voxel_coords": c, "voxel_features1": f.clone(), "voxel_coords1": c.clone(), "batch_size": len(clouds),
                "gt_boxes": gt, "css_score": css}
    # ground truth where the first stage proposes (training-mode predictions do not depend on the targets): a first pass picks RoIs
    scene_gt = torch.zeros((2, 10, 8), device="cuda")
    scene_gt[:, 0] = torch.tensor([5.0, 5.0, 0.5, 4.5, 2.0, 1.6, 0.3, 1.0])
    css = torch.linspace(0.2, 1.0, 10, device="cuda").repeat(2, 1)
    css[:, 3] = 0.0
    with torch.no_grad():
        bd = batch(scene_gt)
        for m in net.module_list[:-1]:
            bd = m(bd)
    rois, labels = bd["rois"], bd["roi_labels"]
    pick = torch.linspace(0, rois.shape[1] - 1, 10, device="cuda").long()
    gt = torch.cat([rois[:, pick], labels[:, pick, None].float()], -1).contiguous()

    def step(fused):
        set_fused_loss(net, fused)
        net.roi_head.iter = 1
        np.random.seed(11)
        torch.manual_seed(11)
        net.zero_grad()
        ret, tb, _ = net(batch(gt))
        return ret["loss"], tb
    want, tb_want = step(False)
    with ops.launch_log() as log:
        got, tb_got = step(True)
    assert log.counts.get("rcnn_proto_loss_kernel") == 1, log.counts
    assert bool(torch.isfinite(got)) and abs(float(got) - float(want)) <= 2e-4 * abs(float(want)), (float(got), float(want))
    assert abs(tb_got["rcnn_loss"] - tb_want["rcnn_loss"]) <= 2e-4 * abs(tb_want["rcnn_loss"]), (tb_got["rcnn_loss"], tb_want["rcnn_loss"])
    assert float(net.roi_head.last_losses[11]) > 0, "no foreground RoI: the comparison would say little"
    got.backward()
    for k, p in net.roi_head.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
