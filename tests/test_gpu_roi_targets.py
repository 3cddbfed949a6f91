"""GPU: the device proposal-target layer (csrc/roi_targets.hip: cpd_roi_targets_classify / cpd_roi_targets_gather, behind
ProposalTargetLayer.fused) against the torch path of cpd_amd.roi_head_train under equal seeds, and against the reference's own
fixtures (proto_head.npz, voxel_rcnn_head_train.npz, target_layer_x.npz) at the tolerances of the existing tests of those fixtures.

Everything that is a gather, a comparison or one IEEE operation is compared exactly. The canonical gt_of_rois (sin / cos / mod) and
the direction weight of roi_ioud* are compared with the torch formulas evaluated in float64 on the same sampled rows: the device
result may lie no farther from that than twice the torch-fp32 path's own largest distance on the case, or one fp32 ulp of the value."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi


# ---------------------------------------------------------------------------------------------------------------- scenes
def _boxes(gen, k, spread=40.0):
    r = lambda *s: torch.rand(*s, generator=gen)
    return torch.cat([(r(k, 2) - 0.5) * spread, r(k, 1) - 0.5, 1.5 + 3 * r(k, 1), 1.0 + 1.5 * r(k, 1), 1.2 + 0.8 * r(k, 1), (r(k, 1) - 0.5) * 7.0], 1)


def _gt_frames(gen, m=130):
    """Five frames of [m, 8] ground truth (class in the last column), one per layout: one real row; only zero rows; a zero row
    between real rows; 65 rows; 130 rows (both cross the 64-row LDS tile). The 65-row frame holds two identical rows (20, 21) and
    no class 3; the others draw classes 1..3."""
    out = torch.zeros(5, m, 8)
    for f, k in ((0, 1), (2, 5), (3, 65), (4, 130)):
        out[f, :k, :7] = _boxes(gen, k)
        out[f, :k, 7] = torch.randint(1, 3 if f == 3 else 4, (k,), generator=gen).float()
    out[2, 2] = 0
    out[3, 21] = out[3, 20]
    return out


def _rois(gen, gt, n, dup):
    """n RoIs per frame: 0 = disjoint from everything, 1 = identical to `dup` (the 65-row frame's duplicated rows), the last tenth zero padding (as the
    proposal NMS leaves it), the rest jittered copies of ground-truth rows; labels mostly the row's class, some of a class the frame
    lacks, some outside 1..3."""
    b, m = gt.shape[:2]
    rois, labels = torch.zeros(b, n, 7), torch.ones(b, n, dtype=torch.long)
    for f in range(b):
        src = gt[f, torch.randint(0, m, (n,), generator=gen)]
        real = src[:, 3] > 0
        box = src[:, :7] + torch.randn(n, 7, generator=gen) * torch.tensor([0.3, 0.3, 0.1, 0.2, 0.1, 0.1, 0.15])
        box[~real] = _boxes(gen, int((~real).sum()))
        lab = torch.where(real, src[:, 7].long(), torch.randint(1, 4, (n,), generator=gen))
        odd = torch.rand(n, generator=gen)
        lab = torch.where(odd < 0.1, torch.randint(1, 4, (n,), generator=gen), lab)
        lab = torch.where(odd > 0.95, torch.tensor([0, 7])[torch.randint(0, 2, (n,), generator=gen)], lab)
        rois[f], labels[f] = box, lab
        rois[f, 0] = torch.tensor([500.0, 500.0, 0.0, 4.0, 2.0, 1.5, 0.3])
        labels[f, 0] = 1
        if n > 1:
            rois[f, 1], labels[f, 1] = dup[:7], int(dup[7])
        pad = n // 10
        if pad:
            rois[f, n - pad:] = 0
    return rois, labels


def _torch_classify(layer, rois, labels, gt, by_class):
    """sample_rois_for_rcnn's trimming and overlaps, frame by frame (the torch path)"""
    from cpd_amd import ops
    out = []
    for i in range(rois.shape[0]):
        cur = gt[i]
        nz = (cur.sum(1) != 0).nonzero()
        k = int(nz[-1]) if nz.numel() else 0
        cur = cur[:k + 1]
        if by_class:
            ov, asg = layer.get_max_iou_with_same_class(rois[i], labels[i], cur[:, 0:7], cur[:, -1].long())
        else:
            ov, asg = torch.max(ops.boxes_iou3d(rois[i][:, 0:7].contiguous(), cur[:, 0:7].contiguous()), dim=1)
        out.append((ov, asg, cur))
    return out


def _torch_pools(ov, cfg, gts):
    lo = cfg["CLS_BG_THRESH_LO"]
    easy = ov < lo
    if gts is None:
        fg = ov >= min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])
        hard = (ov < cfg["REG_FG_THRESH"]) & (ov >= lo)
    else:
        fg, hard = torch.zeros_like(easy), torch.zeros_like(easy)
        for c, (r, k) in enumerate(zip(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])):
            own = gts[..., -1] == (c + 1)
            fg |= (ov >= min(r, k)) & own
            hard |= (ov < r) & (ov >= lo) & own
    return [m.nonzero().view(-1) for m in (fg, hard, easy)]


SCALAR = dict(CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, REG_FG_THRESH=0.55)
LISTS = dict(CLS_FG_THRESH=[0.75, 0.6, 0.65], CLS_BG_THRESH=[0.25, 0.15, 0.2], CLS_BG_THRESH_LO=0.1, REG_FG_THRESH=[0.55, 0.4, 0.45])


@pytest.fixture(scope="module")
def scene(hip):
    """the five ground-truth frames, on the device and on the host"""
    gt = _gt_frames(torch.Generator().manual_seed(2024))
    return gt.cuda(), gt


# ---------------------------------------------------------------------------------------------------------------- classify
@pytest.mark.parametrize("by_class", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 512])
def test_classify_matches_torch_path(scene, n, by_class):
    from cpd_amd import ops
    from cpd_amd.roi_head_train import ProposalTargetLayer
    gt, gt_host = scene
    rois, labels = (t.cuda() for t in _rois(torch.Generator().manual_seed(1000 + n), gt_host, n, gt_host[3, 20]))
    want = _torch_classify(ProposalTargetLayer(SCALAR), rois, labels, gt, by_class)
    for cfg in (SCALAR, LISTS):
        lists = isinstance(cfg["REG_FG_THRESH"], list)
        fg_t = [min(r, c) for r, c in zip(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])] if lists else min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])
        ws = torch.zeros(int(ops.lib().cpd_roi_targets_workspace_bytes(gt.shape[0], n)), dtype=torch.uint8, device="cuda")
        counts, _ = ops.roi_targets_classify(rois, labels, gt, by_class, fg_t, cfg["REG_FG_THRESH"], cfg["CLS_BG_THRESH_LO"], workspace=ws)
        ov, asg, pools = ops.roi_targets_views(ws, gt.shape[0], n)
        cnt = counts.cpu().tolist()
        for f, (w_ov, w_asg, cur) in enumerate(want):
            assert torch.equal(ov[f].view(torch.int32), w_ov.view(torch.int32)), (f, n, by_class)           # bit-equal
            assert torch.equal(asg[f].long(), w_asg), (f, n, by_class)
            assert cnt[f][3] == cur.shape[0] == (1, 1, 5, 65, 130)[f]
            for p, w_list in enumerate(_torch_pools(w_ov, cfg, cur[w_asg] if lists else None)):
                assert cnt[f][p] == w_list.numel(), (f, p, cnt[f], w_list.numel())
                assert torch.equal(pools[p][f, :cnt[f][p]].long(), w_list), (f, p)
        # two calls agree bit for bit
        ws2 = torch.zeros_like(ws)
        counts2, _ = ops.roi_targets_classify(rois, labels, gt, by_class, fg_t, cfg["REG_FG_THRESH"], cfg["CLS_BG_THRESH_LO"], workspace=ws2)
        assert torch.equal(ws, ws2) and torch.equal(counts, counts2)
    # the tie rule, shown and not assumed: the disjoint RoI overlaps nothing -- in the by-class mode it is assigned the first row of
    # its own class (where the frame has one), otherwise row 0; the RoI identical to rows 20 and 21 of frame 3 gets row 20
    for f, (w_ov, w_asg, cur) in enumerate(want):
        assert float(w_ov[0]) == 0.0
        own = (cur[:, -1].long() == labels[f, 0]).nonzero().view(-1)
        assert int(w_asg[0]) == (int(own[0]) if by_class and own.numel() else 0)
    if n > 1:
        assert int(want[3][1][1]) == 20 and float(want[3][0][1]) > 0.99
        assert float(want[1][0].abs().max()) == 0.0 and int(want[1][1].abs().max()) == 0        # the all-zero frame: one zero row kept


# ---------------------------------------------------------------------------------------------------------------- gather / layer
def _cfg(kind, per_image, hard):
    base = dict(LISTS if kind.endswith("_x") else SCALAR)
    base.update(ROI_PER_IMAGE=per_image, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE=kind, HARD_BG_RATIO=0.8,
                DIRECTION_MIN=0.1, DIRECTION_MAX=0.9, ENABLE_HARD_SAMPLING=hard, HARD_SAMPLING_THRESH=[0.3, 0.2, 0.25],
                HARD_SAMPLING_RATIO=[0.5, 0.25, 0.34])
    return base


def _limit64(a):
    a = np.mod(a, TWO_PI)
    a = np.where(a > np.pi, a - TWO_PI, a)
    return np.where(a < -np.pi, a + TWO_PI, a)


def _canonical64(rois, src):
    """assign_targets' transformation (roi_head_template.py:124-145) in float64"""
    rois, gt = rois.astype(np.float64), src.astype(np.float64).copy()
    ry = np.mod(rois[..., 6], TWO_PI)
    gt[..., 0:3] -= rois[..., 0:3]
    gt[..., 6] -= ry
    c, s = np.cos(-ry), np.sin(-ry)
    x, y = gt[..., 0].copy(), gt[..., 1].copy()
    gt[..., 0], gt[..., 1] = x * c - y * s, x * s + y * c
    h = np.mod(gt[..., 6], TWO_PI)
    h = np.where((h > np.pi * 0.5) & (h < np.pi * 1.5), np.mod(h + np.pi, TWO_PI), h)
    h = np.where(h > np.pi, h - TWO_PI, h)
    gt[..., 6] = np.clip(h, -np.pi / 2, np.pi / 2)
    return gt


def _labels64(cfg, rois, src, iou):
    """the roi_ioud / roi_ioud_x soft labels (proposal_target_layer.py:100-184) in float64 on the fp32 overlaps"""
    rois, src, iou = rois.astype(np.float64), src.astype(np.float64), iou.astype(np.float64)
    d = np.abs(_limit64(rois[..., 6]) - _limit64(src[..., 6]))
    w = 1 - np.minimum(d, TWO_PI - d) / np.pi
    lo, hi = cfg["DIRECTION_MIN"], cfg["DIRECTION_MAX"]
    dw = (np.clip(w, lo, hi) - lo) / (hi - lo)

    def soft(fg_t, bg_t):
        # the comparisons as the fp32 paths make them: against the threshold cast to float
        fg, bg = iou > np.float32(fg_t), iou < np.float32(bg_t)
        return np.where(fg, 1.0, np.where(bg, 0.0, (iou - bg_t) / (fg_t - bg_t))) * dw
    if cfg["CLS_SCORE_TYPE"] == "roi_ioud":
        return soft(cfg["CLS_FG_THRESH"], cfg["CLS_BG_THRESH"])
    out = np.zeros_like(iou)
    for c, (f, b) in enumerate(zip(cfg["CLS_FG_THRESH"], cfg["CLS_BG_THRESH"])):
        out = np.where(src[..., -1] == c + 1, soft(f, b), out)
    return out


def _within(dev, fp32, y64, what):
    """|dev - y64| <= max(2 x the torch-fp32 path's largest distance on this case, one fp32 ulp of the value)"""
    dev, fp32 = dev.double().cpu().numpy(), fp32.double().cpu().numpy()
    d_torch, d_dev = float(np.abs(fp32 - y64).max()), float(np.abs(dev - y64).max())
    print("%s: largest distance from float64  torch-fp32 %.3e  device %.3e" % (what, d_torch, d_dev))
    bound = np.maximum(2 * d_torch, np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64))
    assert bool((np.abs(dev - y64) <= bound).all()), (what, d_torch, d_dev)
    return d_torch, d_dev


KINDS = ("cls", "roi_iou", "roi_ioud", "roi_iou_x", "roi_ioud_x")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,per_image", [(1, 8), (2, 24), (3, 130)])
def test_layer_matches_torch_path_under_equal_seeds(scene, b, per_image, kind):
    from cpd_amd import ops
    from cpd_amd.roi_head_train import ProposalTargetLayer, assign_targets
    gt_all, gt_host = scene
    gen = torch.Generator().manual_seed(50 * b + KINDS.index(kind))
    gt = gt_all[[4, 2, 3][:b]].contiguous()
    rois, labels = (t.cuda() for t in _rois(gen, gt_host[[4, 2, 3][:b]], 200, gt_host[3, 20]))
    extras = (b + KINDS.index(kind)) % 2 == 0                          # present in half of the cases
    cfg = _cfg(kind, per_image, hard=kind.endswith("_x") and b != 2)
    bd = {"batch_size": b, "rois": rois, "roi_labels": labels, "roi_scores": torch.rand(b, 200, generator=gen).cuda(), "gt_boxes": gt}
    if extras:
        for key in ("css_score", "outline_cls_mask", "outline_reg_mask"):
            bd[key] = torch.rand(b, gt.shape[1], generator=gen).cuda()
    layer = ProposalTargetLayer(cfg)
    seed = 31 + 7 * b + KINDS.index(kind)

    def run(fused):
        layer.fused = fused
        np.random.seed(seed)
        torch.manual_seed(seed)
        with ops.launch_log() as log:
            t = assign_targets(layer, dict(bd))
        return t, log.counts, (np.random.rand(), float(torch.rand(1)))
    want, _, tail_want = run(False)
    got, counts, tail_got = run(True)
    assert counts == {"roi_targets_classify_kernel": 1, "roi_targets_gather_kernel": 1}, counts          # whatever b is
    assert tail_got == tail_want                                       # the same numbers were drawn
    assert sorted(got) == sorted(want) and sorted(got["additional_data"]) == sorted(want["additional_data"])
    assert len(got["additional_data"]) == (3 if extras else 0)
    for k in want:
        if k != "additional_data":
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].device == want[k].device, k
    exact = ["rois", "roi_labels", "roi_scores", "gt_iou_of_rois", "gt_of_rois_src", "reg_valid_mask"]
    if kind in ("cls", "roi_iou", "roi_iou_x"):
        exact.append("rcnn_cls_labels")
    for k in exact:
        assert torch.equal(got[k], want[k]), k
    for k in want["additional_data"]:
        assert torch.equal(got["additional_data"][k], want["additional_data"][k]), k
    assert int(want["reg_valid_mask"].sum()) > 0 and int((want["reg_valid_mask"] == 0).sum()) > 0
    r, s, iou = (want[k].cpu().numpy() for k in ("rois", "gt_of_rois_src", "gt_iou_of_rois"))
    _within(got["gt_of_rois"], want["gt_of_rois"], _canonical64(r, s), "gt_of_rois %s b=%d" % (kind, b))
    if kind in ("roi_ioud", "roi_ioud_x"):
        _within(got["rcnn_cls_labels"], want["rcnn_cls_labels"], _labels64(cfg, r, s, iou), "rcnn_cls_labels %s b=%d" % (kind, b))


# ---------------------------------------------------------------------------------------------------------------- the reference's goldens
def _pool_cfg():
    return dict(FEATURES_SOURCE=["x_conv3", "x_conv4"], PRE_MLP=True, GRID_SIZE=2, POOL_LAYERS=dict(
        x_conv3=dict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[0.6, 1.2], NSAMPLE=[8, 8], POOL_METHOD="max_pool"),
        x_conv4=dict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[1.2, 2.4], NSAMPLE=[8, 8], POOL_METHOD="max_pool")))


def _head_cfg(proto):
    """the model_cfg of tests/test_gpu_roi_train.py (proto) / tests/test_gpu_rcnn_head_train.py"""
    weights = dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8])
    cfg = dict(
        CLASS_AGNOSTIC=True, ROI_GRID_POOL=_pool_cfg(), SHARED_FC=[48, 48], CLS_FC=[32, 32], REG_FC=[32, 32], DP_RATIO=0.0,
        TARGET_CONFIG=dict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=24, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou",
                           CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.02, CLS_BG_THRESH_LO=0.01, HARD_BG_RATIO=0.1, REG_FG_THRESH=0.3),
        LOSS_CONFIG=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True, GRID_3D_IOU_LOSS=False,
                         LOSS_WEIGHTS=weights),
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=400, NMS_POST_MAXSIZE=60, NMS_THRESH=0.8)))
    if proto:
        cfg["ROI_GRID_POOL_PROTO"] = _pool_cfg()
        weights.update(rcnn_proto_weight=1.0, rcnn_iou3d_weight=1.0)
    return cfg


def _close(got, want, what, rtol=2e-4, floor=2e-5):                   # tests/test_gpu_roi_train.py::_close
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-12)
    err = float(np.abs(got - want).max())
    assert err <= rtol * scale + floor, "%s: max |diff| %.3e vs scale %.3e" % (what, err, scale)


def _close_rel(got, want, what, rtol=2e-4, floor=2e-5):               # tests/test_gpu_rcnn_head_train.py::_close
    scale = max(float(np.abs(want).max()), floor)
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    assert err <= rtol * scale, "%s: max err %g vs scale %g" % (what, err, scale)


def _levels(g, keys, grad=True):
    out = [{} for _ in keys]
    for name, shp in (("x_conv3", [11, 104, 104]), ("x_conv4", [5, 52, 52])):
        idx = torch.from_numpy(g[name + "_idx"]).cuda()
        for d, key in zip(out, keys):
            f = torch.from_numpy(g[name + key]).cuda().requires_grad_(grad)
            d[name] = types.SimpleNamespace(indices=idx, features=f, spatial_shape=shp, batch_size=2)
    return out


def _check_sampled_targets(t, g, extra=None):
    """the sampling / target block of the existing fixture tests, at their tolerances; what the sampler selects is exact"""
    np.testing.assert_allclose(t["rois"].cpu().numpy(), g["t_rois"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(t["roi_labels"].cpu().numpy(), g["t_roi_labels"])
    np.testing.assert_array_equal(t["reg_valid_mask"].cpu().numpy(), g["t_reg_valid_mask"])
    np.testing.assert_allclose(t["gt_iou_of_rois"].cpu().numpy(), g["t_gt_iou_of_rois"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(t["rcnn_cls_labels"].cpu().numpy(), g["t_rcnn_cls_labels"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(t["gt_of_rois"].cpu().numpy(), g["t_gt_of_rois"], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(t["gt_of_rois_src"].cpu().numpy(), g["t_gt_of_rois_src"])
    assert int((t["reg_valid_mask"] > 0).sum()) > 0


def test_proto_head_golden_with_the_switch_on(golden, hip):
    from cpd_amd import ops
    from cpd_amd.roi_head_train import VoxelRCNNProtoHead, set_fused_targets
    g = golden("proto_head")
    head = VoxelRCNNProtoHead(input_channels={"x_conv3": 8, "x_conv4": 12}, model_cfg=_head_cfg(True), point_cloud_range=g["pcr"].tolist(),
                              voxel_size=[0.1, 0.1, 0.15], num_class=1)
    head.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("h.")}, strict=True)
    head = head.cuda().train()
    assert set_fused_targets(head) == 1
    lv, lv_mm = _levels(g, ("_feat", "_feat_mm"))
    bd = {"batch_size": 2, "batch_box_preds": torch.from_numpy(g["boxes"]).cuda(), "batch_cls_preds": torch.from_numpy(g["cls"]).cuda(),
          "gt_boxes": torch.from_numpy(g["gt"]).cuda(), "css_score": torch.from_numpy(g["css"]).cuda(), "multi_scale_3d_features": lv,
          "multi_scale_3d_features_mm": lv_mm, "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    with ops.launch_log() as log:
        head(bd)
    # one head forward: exactly two target launches
    assert {k: v for k, v in log.counts.items() if k.startswith("roi_targets")} == {"roi_targets_classify_kernel": 1,
                                                                                  "roi_targets_gather_kernel": 1}, log.counts
    t0, t1 = head.forward_ret_dict["targets_dict0"], head.forward_ret_dict["targets_dict1"]
    _check_sampled_targets(t0, g)
    np.testing.assert_array_equal(t0["additional_data"]["css_score"].cpu().numpy(), g["t_css"])
    np.testing.assert_allclose(t0["roi_scores"].cpu().numpy(), g["t_roi_scores"], rtol=0, atol=1e-6)
    for i, t in enumerate((t0, t1)):
        for k in ("shared_features", "rcnn_cls", "rcnn_reg"):
            _close(t[k].detach().cpu().numpy(), g["o%d_%s" % (i, k)], "branch %d %s" % (i, k))
    loss, tb = head.get_loss()
    assert abs(loss.item() - float(g["loss"])) <= 2e-4 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))
    assert abs(tb["rcnn_loss"] - float(g["rcnn_loss"])) <= 2e-4 * abs(float(g["rcnn_loss"]))
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


def test_voxel_rcnn_head_golden_with_the_switch_on(golden, hip):
    from cpd_amd import ops, roi_pool
    from cpd_amd.roi_head_train import set_fused_targets
    g = golden("voxel_rcnn_head_train")
    head = roi_pool.VoxelRCNNHead(input_channels={"x_conv3": 8, "x_conv4": 12}, model_cfg=_head_cfg(False), point_cloud_range=g["pcr"].tolist(),
                                  voxel_size=[0.1, 0.1, 0.15], num_class=1)
    head.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("h.")}, strict=True)
    head = head.cuda().train()
    assert set_fused_targets(head) == 1
    lv, = _levels(g, ("_feat",))
    bd = {"batch_size": 2, "batch_box_preds": torch.from_numpy(g["boxes"]).cuda(), "batch_cls_preds": torch.from_numpy(g["cls"]).cuda(),
          "gt_boxes": torch.from_numpy(g["gt"]).cuda(), "multi_scale_3d_features": lv, "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    with ops.launch_log() as log:
        head(bd)
    assert {k: v for k, v in log.counts.items() if k.startswith("roi_targets")} == {"roi_targets_classify_kernel": 1,
                                                                                  "roi_targets_gather_kernel": 1}, log.counts
    t = head.forward_ret_dict
    _check_sampled_targets(t, g)
    for k in ("rcnn_cls", "rcnn_reg"):
        _close_rel(t[k].detach().cpu().numpy(), g["o_" + k], k)
    t["rcnn_cls"].retain_grad()
    t["rcnn_reg"].retain_grad()
    loss, tb = head.get_loss()
    want_loss = float(g["loss"])
    assert abs(loss.item() - want_loss) <= 2e-4 * abs(want_loss), (loss.item(), want_loss)
    for k, v in zip(g["tb_keys"].tolist(), g["tb_values"].tolist()):
        assert abs(tb[k] - v) <= 2e-4 * abs(v) + 1e-7, (k, tb[k], v)
    loss.backward()
    _close_rel(t["rcnn_cls"].grad.cpu().numpy(), g["d_rcnn_cls"], "d loss / d rcnn_cls", rtol=1e-3, floor=1e-7)
    _close_rel(t["rcnn_reg"].grad.cpu().numpy(), g["d_rcnn_reg"], "d loss / d rcnn_reg", rtol=1e-3, floor=1e-7)
    params = dict(head.named_parameters())
    n = 0
    for k in g.files:
        if k.startswith("g."):
            _close_rel(params[k[2:]].grad.cpu().numpy(), g[k], "grad " + k[2:], rtol=1e-3, floor=1e-6)
            n += 1
    assert n >= 20
    for name in ("x_conv3", "x_conv4"):
        _close_rel(lv[name].features.grad.cpu().numpy()[::4], g[name + "_grad4"], "d loss / d " + name, rtol=1e-3, floor=1e-7)


def test_per_class_threshold_golden_with_the_switch_on(golden, hip):
    """tests/test_gpu_roi_train.py::test_per_class_threshold_target_layer_matches_reference through the device path."""
    from cpd_amd.roi_head_train import ProposalTargetLayer
    g = golden("target_layer_x")
    bd = {"batch_size": 2, "rois": torch.from_numpy(g["rois"]).cuda(), "roi_scores": torch.from_numpy(g["roi_scores"]).cuda(),
          "roi_labels": torch.from_numpy(g["roi_labels"]).cuda(), "gt_boxes": torch.from_numpy(g["gt"]).cuda()}
    for case in range(int(g["n_cases"])):
        pre = "c%d_" % case
        cfg = dict(ROI_PER_IMAGE=64, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE=("roi_iou_x", "roi_ioud_x")[int(g[pre + "kind"])],
                   CLS_FG_THRESH=[0.75, 0.6, 0.65], CLS_BG_THRESH=[0.25, 0.15, 0.2], CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8,
                   REG_FG_THRESH=[0.55, 0.4, 0.45], DIRECTION_MIN=0.1, DIRECTION_MAX=0.9, ENABLE_HARD_SAMPLING=bool(g[pre + "hard"]),
                   HARD_SAMPLING_THRESH=[0.3, 0.2, 0.25], HARD_SAMPLING_RATIO=[0.5, 0.25, 0.34])
        np.random.seed(int(g[pre + "seed"]))
        torch.manual_seed(int(g[pre + "seed"]))
        layer = ProposalTargetLayer(cfg)
        layer.fused = True
        assert layer.fused_ok(bd)
        t = layer(dict(bd))
        np.testing.assert_array_equal(t["rois"].cpu().numpy(), g[pre + "rois"], err_msg=pre)
        np.testing.assert_array_equal(t["gt_of_rois"].cpu().numpy(), g[pre + "gt_of_rois"], err_msg=pre)
        np.testing.assert_array_equal(t["roi_labels"].cpu().numpy(), g[pre + "roi_labels"], err_msg=pre)
        np.testing.assert_array_equal(t["roi_scores"].cpu().numpy(), g[pre + "roi_scores"], err_msg=pre)
        np.testing.assert_array_equal(t["reg_valid_mask"].cpu().numpy(), g[pre + "reg_valid_mask"], err_msg=pre)
        np.testing.assert_allclose(t["gt_iou_of_rois"].cpu().numpy(), g[pre + "gt_iou_of_rois"], rtol=0, atol=1e-5, err_msg=pre)
        np.testing.assert_allclose(t["rcnn_cls_labels"].cpu().numpy(), g[pre + "rcnn_cls_labels"], rtol=0, atol=5e-5, err_msg=pre)
        assert int(t["reg_valid_mask"].sum()) > 20 and 0.0 < float(t["rcnn_cls_labels"].mean()) < 1.0
