"""GPU: training of the anchor-head VoxelRCNN's RoI head (voxel_rcnn_dbscan / oyster configs) -- the fused loss-and-gradient
kernel `cpd_rcnn_loss` against its torch restatement, VoxelRCNNHead's training step against the reference's
(tests/golden/voxel_rcnn_head_train.npz), the eval FC cache after an optimizer step, and the detector's training forward end to end."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _head_cfg():
    pool = dict(FEATURES_SOURCE=["x_conv3", "x_conv4"], PRE_MLP=True, GRID_SIZE=2, POOL_LAYERS=dict(
        x_conv3=dict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[0.6, 1.2], NSAMPLE=[8, 8], POOL_METHOD="max_pool"),
        x_conv4=dict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[1.2, 2.4], NSAMPLE=[8, 8], POOL_METHOD="max_pool")))
    return dict(
        CLASS_AGNOSTIC=True, ROI_GRID_POOL=pool, SHARED_FC=[48, 48], CLS_FC=[32, 32], REG_FC=[32, 32], DP_RATIO=0.0,
        TARGET_CONFIG=dict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=24, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou",
                           CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.02, CLS_BG_THRESH_LO=0.01, HARD_BG_RATIO=0.1, REG_FG_THRESH=0.3),
        LOSS_CONFIG=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True, GRID_3D_IOU_LOSS=False,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0,
                                           code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8])),
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=400, NMS_POST_MAXSIZE=60, NMS_THRESH=0.8)))


def _close(got, want, what, rtol=2e-4, floor=2e-5):
    scale = max(float(np.abs(want).max()), floor)
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    assert err <= rtol * scale, "%s: max err %g vs scale %g" % (what, err, scale)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _args(t, dev="cuda"):
    return [torch.as_tensor(t[k]).to(dev) for k in ("rcnn_cls", "rcnn_reg", "rois", "gt_of_rois", "gt_of_rois_src", "reg_valid_mask",
                                                    "rcnn_cls_labels")]


def _fixture_case(g, i):
    p = "c%d_" % i
    t = {k: g[p + k] for k in ("rcnn_cls", "rcnn_reg", "rois", "gt_of_rois", "gt_of_rois_src", "reg_valid_mask", "rcnn_cls_labels")}
    w = g[p + "weights"]
    return t, dict(code_weights=g[p + "code_weights"].tolist(), cls_weight=float(w[0]), reg_weight=float(w[1]), corner_weight=float(w[2]),
                   corner_regularization=bool(g[p + "corner_reg"]))


def _random_case(n, seed):
    """n rows: RoIs with headings across the circle (some near +-pi/2 and pi), canonical gt near the RoI frame's origin, source gt
    sometimes turned by pi, logits with saturated ones, fractional / 0 / 1 / -1 labels, about half foreground."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen)
    nrm = lambda *s: torch.randn(*s, generator=gen)
    rois = torch.cat([(r(n, 2) - 0.5) * 60, r(n, 1) - 0.5, 0.6 + 4 * r(n, 3), (r(n, 1) - 0.5) * 6.4], 1)
    edge = r(n) < 0.3
    rois[edge, 6] = torch.tensor([np.pi / 2, -np.pi / 2, np.pi, -np.pi])[torch.randint(0, 4, (int(edge.sum()),), generator=gen)]
    gt_ct = torch.cat([nrm(n, 3) * 0.4, rois[:, 3:6] * (0.8 + 0.45 * r(n, 3)), (r(n, 1) - 0.5) * 3.0, torch.ones(n, 1)], 1)
    src = torch.cat([rois[:, 0:3] + nrm(n, 3) * 0.4, gt_ct[:, 3:6], rois[:, 6:7] + nrm(n, 1) * 0.2 + np.pi * (r(n, 1) < 0.3).float(),
                     torch.ones(n, 1)], 1)
    cls = nrm(n, 1) * 4
    sat = r(n) < 0.1
    cls[sat, 0] = torch.tensor([20.0, -20.0, 40.0, -40.0])[torch.randint(0, 4, (int(sat.sum()),), generator=gen)]
    reg = nrm(n, 7) * 0.3
    lab = torch.where(r(n) < 0.4, r(n), (r(n) < 0.5).float())
    lab[r(n) < 0.15] = -1.0
    mask = (r(n) < 0.5).long()
    t = dict(rcnn_cls=cls, rcnn_reg=reg, rois=rois.view(1, n, 7), gt_of_rois=gt_ct.view(1, n, 8), gt_of_rois_src=src.view(1, n, 8),
             reg_valid_mask=mask.view(1, n), rcnn_cls_labels=lab.view(1, n))
    return t, dict(code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8], cls_weight=1.0, reg_weight=1.0, corner_weight=1.0,
                   corner_regularization=True)


def _check_against_restatement(t, kw, what):
    from cpd_amd.roi_head_train import rcnn_head_loss_torch, rcnn_loss_fused
    args = _args(t)
    cls = args[0].clone().requires_grad_(True)
    reg = args[1].clone().requires_grad_(True)
    total, terms = rcnn_head_loss_torch(cls, reg, *args[2:], **kw)
    total.backward()
    losses, d_cls, d_reg = rcnn_loss_fused(*args, **kw)
    lv = losses.cpu().numpy().astype(np.float64)
    value = lambda v: float(v.item()) if torch.is_tensor(v) else float(v)
    want = [value(total), value(terms["rcnn_loss_cls"]), value(terms["rcnn_loss_reg"]), value(terms.get("rcnn_loss_corner", 0.0)),
            value(terms["rcnn_loss_bb"]), value(terms["fg"])]
    for k, (a, b) in enumerate(zip(lv, want)):
        assert abs(a - b) <= 1e-5 * abs(b) + 1e-7, (what, k, a, b)
    for got, ref, name in ((d_cls, cls.grad, "d_cls"), (d_reg, reg.grad, "d_reg")):
        assert got.shape == ref.shape
        err = float((got - ref).abs().max()) if ref.numel() else 0.0
        assert err <= 1e-5 * float(ref.abs().max()) + 1e-7, (what, name, err, float(ref.abs().max()))
    # deterministic: a second call is bitwise equal
    losses2, d_cls2, d_reg2 = rcnn_loss_fused(*args, **kw)
    assert torch.equal(losses, losses2) and torch.equal(d_cls, d_cls2) and torch.equal(d_reg, d_reg2), what
    return terms


@pytest.mark.parametrize("i", range(6))
def test_fused_rcnn_loss_matches_restatement_on_reference_cases(golden, hip, i):
    g = golden("rcnn_loss")
    t, kw = _fixture_case(g, i)
    terms = _check_against_restatement(t, kw, str(g["names"][i]))
    assert abs(float(terms["rcnn_loss_cls"]) + float(terms["rcnn_loss_reg"]) + float(terms.get("rcnn_loss_corner", 0.0))
               + float(terms["rcnn_loss_bb"]) - float(g["c%d_total" % i])) <= 2e-5 * abs(float(g["c%d_total" % i]))


@pytest.mark.parametrize("n", [1, 63, 300, 4096])
def test_fused_rcnn_loss_matches_restatement_on_random_rows(hip, n):
    t, kw = _random_case(n, seed=100 + n)
    _check_against_restatement(t, kw, "n=%d" % n)


def test_fused_rcnn_loss_without_rows_writes_zero_losses(hip):
    from cpd_amd.roi_head_train import rcnn_loss_fused
    z = lambda *s: torch.zeros(*s, device="cuda")
    losses, d_cls, d_reg = rcnn_loss_fused(z(0, 1), z(0, 7), z(1, 0, 7), z(1, 0, 8), z(1, 0, 8), z(1, 0), z(1, 0), [1.0] * 7)
    assert losses.shape == (6,) and float(losses.abs().sum()) == 0.0
    assert d_cls.shape == (0, 1) and d_reg.shape == (0, 7)


# ---------------------------------------------------------------------------------------------------------------- the head
def _fixture_head(g):
    from cpd_amd import roi_pool
    head = roi_pool.VoxelRCNNHead(input_channels={"x_conv3": 8, "x_conv4": 12}, model_cfg=_head_cfg(), point_cloud_range=g["pcr"].tolist(),
                                  voxel_size=[0.1, 0.1, 0.15], num_class=1)
    head.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("h.")}, strict=True)
    return head.cuda()


def _fixture_batch(g, grad=True):
    lv = {}
    for name, shp in (("x_conv3", [11, 104, 104]), ("x_conv4", [5, 52, 52])):
        f = torch.from_numpy(g[name + "_feat"]).cuda().requires_grad_(grad)
        lv[name] = types.SimpleNamespace(indices=torch.from_numpy(g[name + "_idx"]).cuda(), features=f, spatial_shape=shp, batch_size=2)
    return {"batch_size": 2, "batch_box_preds": torch.from_numpy(g["boxes"]).cuda(), "batch_cls_preds": torch.from_numpy(g["cls"]).cuda(),
            "gt_boxes": torch.from_numpy(g["gt"]).cuda(), "multi_scale_3d_features": lv, "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}


def test_voxel_rcnn_head_training_step_matches_reference(golden, hip):
    from cpd_amd import ops
    g = golden("voxel_rcnn_head_train")
    head = _fixture_head(g).train()
    bd = _fixture_batch(g)
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    head(bd)
    t = head.forward_ret_dict
    np.testing.assert_allclose(t["rois"].cpu().numpy(), g["t_rois"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(t["roi_labels"].cpu().numpy(), g["t_roi_labels"])
    np.testing.assert_array_equal(t["reg_valid_mask"].cpu().numpy(), g["t_reg_valid_mask"])
    np.testing.assert_allclose(t["gt_iou_of_rois"].cpu().numpy(), g["t_gt_iou_of_rois"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(t["rcnn_cls_labels"].cpu().numpy(), g["t_rcnn_cls_labels"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(t["gt_of_rois"].cpu().numpy(), g["t_gt_of_rois"], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(t["gt_of_rois_src"].cpu().numpy(), g["t_gt_of_rois_src"])
    assert int((t["reg_valid_mask"] > 0).sum()) > 0
    for k in ("rcnn_cls", "rcnn_reg"):
        _close(t[k].detach().cpu().numpy(), g["o_" + k], k)
    t["rcnn_cls"].retain_grad()
    t["rcnn_reg"].retain_grad()
    with ops.launch_log() as log:
        loss, tb = head.get_loss()
    assert log.counts == {"rcnn_loss_kernel": 1}, log.counts
    want_loss = float(g["loss"])
    assert abs(loss.item() - want_loss) <= 2e-4 * abs(want_loss), (loss.item(), want_loss)
    assert sorted(tb) == sorted(g["tb_keys"].tolist())
    for k, v in zip(g["tb_keys"].tolist(), g["tb_values"].tolist()):
        assert abs(tb[k] - v) <= 2e-4 * abs(v) + 1e-7, (k, tb[k], v)
    loss.backward()
    _close(t["rcnn_cls"].grad.cpu().numpy(), g["d_rcnn_cls"], "d loss / d rcnn_cls", rtol=1e-3, floor=1e-7)
    _close(t["rcnn_reg"].grad.cpu().numpy(), g["d_rcnn_reg"], "d loss / d rcnn_reg", rtol=1e-3, floor=1e-7)
    params = dict(head.named_parameters())
    n = 0
    for k in g.files:
        if k.startswith("g."):
            _close(params[k[2:]].grad.cpu().numpy(), g[k], "grad " + k[2:], rtol=1e-3, floor=1e-6)
            n += 1
    assert n >= 20
    for name in ("x_conv3", "x_conv4"):
        _close(bd["multi_scale_3d_features"][name].features.grad.cpu().numpy()[::4], g[name + "_grad4"], "d loss / d " + name,
               rtol=1e-3, floor=1e-7)


def test_eval_after_an_optimizer_step_uses_the_new_weights(golden, hip):
    """The eval path packs the FC stacks once (self._fc); a training forward drops the pack, so .eval() after an optimizer step
    predicts what a fresh head with the updated state_dict predicts."""
    from cpd_amd import roi_pool
    g = golden("voxel_rcnn_head_train")
    head = _fixture_head(g)
    rois = torch.from_numpy(g["t_rois"]).cuda()

    def eval_forward(h):
        bd = _fixture_batch(g, grad=False)
        bd["rois"] = rois.clone()
        with torch.no_grad():
            out = h.eval()(bd)
        return out["batch_cls_preds"].clone(), out["batch_box_preds"].clone()
    before = eval_forward(head)                                          # builds the packed FC images
    head.train()
    opt = torch.optim.Adam(head.parameters(), lr=1e-2)
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    head(_fixture_batch(g))
    loss, _ = head.get_loss()
    opt.zero_grad()
    loss.backward()
    opt.step()
    after = eval_forward(head)
    fresh = roi_pool.VoxelRCNNHead(input_channels={"x_conv3": 8, "x_conv4": 12}, model_cfg=_head_cfg(), point_cloud_range=g["pcr"].tolist(),
                                   voxel_size=[0.1, 0.1, 0.15], num_class=1)
    fresh.load_state_dict(head.state_dict(), strict=True)
    want = eval_forward(fresh.cuda())
    assert not torch.allclose(before[0], want[0], atol=1e-4)              # the step did move the predictions
    torch.testing.assert_close(after[0], want[0], rtol=0, atol=1e-6)
    torch.testing.assert_close(after[1], want[1], rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- the detector
def _dbscan_model(seed=7):
    """tests/test_gpu_two_stage.py::_anchor_model's reduced dbscan / oyster VoxelRCNN, in training mode."""
    from cpd_amd import models
    cfg = models.waymo_voxel_rcnn_dbscan_cfg()
    cfg.BACKBONE_2D.NUM_FILTERS, cfg.BACKBONE_2D.NUM_UPSAMPLE_FILTERS, cfg.BACKBONE_2D.LAYER_NUMS = [64, 128], [128, 128], [2, 2]
    torch.manual_seed(seed)
    net = models.VoxelRCNN(cfg, point_cloud_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 4.0]).cuda()
    with torch.no_grad():
        for br in net.dense_head.BRANCHES:
            getattr(net.dense_head, br)[0].weight.normal_(0, (2.0 / (9 * 64)) ** 0.5)
        net.dense_head.conv_cls[3].weight.normal_(0, 0.5)
        net.dense_head.conv_reg[3].weight.normal_(0, 0.02); net.dense_head.conv_dim[3].weight.normal_(0, 0.02)
    net.roi_head.init_weights()
    return net.train()


def _dbscan_batch(net, gt):
    from cpd_amd import ops
    from cpd_amd.synthetic import waymo_cloud
    clouds = []
    for s_ in (0, 1):
        p = waymo_cloud(s_, n_points=40000 + 5000 * s_)
        p[:, :2] *= 0.3
        clouds.append(torch.from_numpy(p).cuda())
    vox = ops.Voxelizer(net.voxel_size, net.point_cloud_range, 5, 5, 1000000)
    _, coords, _, feats, nvox = vox.batch(clouds)
    n = int(nvox[len(clouds)])
    return {"voxel_features": feats[:n].clone(), "voxel_coords": coords[:n].float(), "batch_size": len(clouds), "gt_boxes": gt,
            "points": torch.cat([torch.nn.functional.pad(c, (1, 0), value=float(b)) for b, c in enumerate(clouds)])}


def test_dbscan_voxel_rcnn_trains_end_to_end(hip):
    from cpd_amd import roi_pool as rp
    from cpd_amd.roi_head_train import rcnn_head_loss_torch
    net = _dbscan_model()
    # ground truth where the first stage proposes: training-mode predictions do not depend on the targets, so a first pass picks
    # proposals (and their classes) as the boxes -- the RoI sampler then has foreground to work with
    scene_gt = torch.zeros((2, 3, 8), device="cuda")
    scene_gt[:, 0] = torch.tensor([5.0, 5.0, 0.5, 4.5, 2.0, 1.6, 0.3, 1.0])
    with torch.no_grad():
        bd = _dbscan_batch(net, scene_gt)
        for m in net.module_list[:-1]:
            bd = m(bd)
        nms = net.model_cfg.ROI_HEAD.NMS_CONFIG["TRAIN"]
        rois, _, labels, _ = rp.proposal_layer(bd["batch_box_preds"], bd["batch_cls_preds"], nms["NMS_THRESH"], nms["NMS_PRE_MAXSIZE"],
                                               nms["NMS_POST_MAXSIZE"], first_rows="auto", device_fallback=True)
    pick = torch.arange(0, 60, 6, device="cuda")
    gt = torch.cat([rois[:, pick], labels[:, pick, None].float()], -1).contiguous()
    net.zero_grad()
    ret, tb, disp = net(_dbscan_batch(net, gt))
    assert set(ret) == {"loss"} and disp == {}
    assert set(tb) == {"rpn_loss_cls", "rpn_loss_loc", "rpn_loss_dir", "rpn_loss", "rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss_corner",
                       "rcnn_loss"}, sorted(tb)
    t = net.roi_head.forward_ret_dict
    assert int((t["reg_valid_mask"] > 0).sum()) > 0
    rpn = net.dense_head.get_loss()[0][0]
    rcnn, _ = net.roi_head.get_loss()
    assert abs(float(ret["loss"]) - float(rpn + rcnn)) <= 1e-6 * abs(float(ret["loss"]))
    assert abs(tb["rpn_loss"] + tb["rcnn_loss"] - float(ret["loss"])) <= 1e-5 * abs(float(ret["loss"]))
    # the head's gradients through the kernel equal those through the torch restatement of the same loss
    lw = net.model_cfg.ROI_HEAD.LOSS_CONFIG["LOSS_WEIGHTS"]
    ref, _ = rcnn_head_loss_torch(t["rcnn_cls"], t["rcnn_reg"], t["rois"], t["gt_of_rois"], t["gt_of_rois_src"], t["reg_valid_mask"],
                                  t["rcnn_cls_labels"], lw["code_weights"], lw["rcnn_cls_weight"], lw["rcnn_reg_weight"],
                                  lw["rcnn_corner_weight"], True)
    assert abs(float(ref) - float(rcnn)) <= 1e-5 * abs(float(ref))
    params = [p for p in net.roi_head.parameters() if p.requires_grad]
    g_ref = torch.autograd.grad(ref, params, retain_graph=True)
    g_hip = torch.autograd.grad(rcnn, params, retain_graph=True)
    for a, b in zip(g_hip, g_ref):
        assert float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-12), (float((a - b).abs().max()), float(b.abs().max()))
    ret["loss"].backward()
    for part in ("backbone_3d", "backbone_2d", "dense_head", "roi_head"):
        for k, p in getattr(net, part).named_parameters():
            if p.requires_grad:
                assert p.grad is not None, part + "." + k
                assert bool(torch.isfinite(p.grad).all()), part + "." + k
