"""The two-stage detector of the shipped config (voxel_rcnn_cproto_center.yaml:13 `NAME: VoxelRCNN`): the fused engine
(cpd_amd/two_stage.py) against the drop-in module composition (cpd_amd.models.VoxelRCNN: CenterPoint modules -> CenterHead rois ->
VoxelRCNNProtoHead eval branch -> post_processing), whose pieces are pinned on the reference's own goldens elsewhere
(test_gpu_roi_pool.py: voxel_rcnn_head.npz / roi_pool.npz; test_gpu_decode_nms.py: nms goldens; test_gpu_pipeline.py: stage one vs
the oracle), and post_processing against a plain restatement of detector3d_template.py:222-343."""
import numpy as np
import pytest
import torch

from cpd_amd import models, ops
from cpd_amd.synthetic import waymo_cloud

pytestmark = pytest.mark.gpu


def _model(seed=3):
    cfg = models.waymo_voxel_rcnn_cfg()
    cfg.BACKBONE_2D.NUM_FILTERS, cfg.BACKBONE_2D.NUM_UPSAMPLE_FILTERS, cfg.BACKBONE_2D.LAYER_NUMS = [64, 128], [128, 128], [2, 2]
    cfg.DENSE_HEAD.POST_PROCESSING.POST_CENTER_LIMIT_RANGE = [-20, -20, -2, 20, 20, 4]
    cfg.DENSE_HEAD.POST_PROCESSING.MAX_OBJ_PER_SAMPLE = 100
    torch.manual_seed(seed)
    net = models.VoxelRCNN(cfg, point_cloud_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 4.0]).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.75, 1.25)
                m.weight.uniform_(0.75, 1.25); m.bias.normal_(0, 0.1)
        for stack in (net.roi_head.cls_layers, net.roi_head.reg_layers):       # the reference's N(0, 0.01) output layers give constant
            stack[-1].weight.normal_(0, 0.3); stack[-1].bias.normal_(0, 0.3)   # scores: spread them, so that the final NMS has work
    return net


def _clouds():
    out = []
    for s_ in (0, 1, 2):
        p = waymo_cloud(s_, n_points=40000 + 5000 * s_)
        p[:, :2] *= 0.3
        out.append(torch.from_numpy(p).cuda())
    return out


def _batch_dict(net, clouds):
    vox = ops.Voxelizer(net.voxel_size, net.point_cloud_range, 5, 5, 1000000)
    _, coords, _, feats, nvox = vox.batch(clouds)
    n = int(nvox[len(clouds)])
    return {"voxel_features": feats[:n].clone(), "voxel_coords": coords[:n].float(), "batch_size": len(clouds)}


def _match(a, b, atol):
    """every box of a has a partner in b (same geometry to atol), one to one"""
    assert a["pred_boxes"].shape == b["pred_boxes"].shape, (a["pred_boxes"].shape, b["pred_boxes"].shape)
    x, y = a["pred_boxes"].cpu().numpy(), b["pred_boxes"].cpu().numpy()
    if len(x) == 0:
        return
    j = np.abs(x[:, None, :] - y[None, :, :]).max(-1).argmin(1)
    assert sorted(j.tolist()) == list(range(len(y)))
    np.testing.assert_allclose(x, y[j], atol=atol, rtol=1e-4)
    np.testing.assert_allclose(a["pred_scores"].cpu().numpy(), b["pred_scores"].cpu().numpy()[j], atol=atol)
    np.testing.assert_array_equal(a["pred_labels"].cpu().numpy(), b["pred_labels"].cpu().numpy()[j])


def test_two_stage_engine_matches_the_module_composition(hip):
    from cpd_amd import spconv as sp
    sp.install(conv_math="f32")
    net = _model()
    clouds = _clouds()
    with torch.no_grad():
        want, _, bd = net(_batch_dict(net, clouds))
    assert bd["rois"].shape[1] == max(1, max(int((bd["roi_scores"][b] > 0).sum()) for b in range(3)))
    ecfg = net.to_engine_config()
    ecfg.conv_math = "f32"
    eng = net.to_engine()
    eng_f32 = type(eng)(ecfg, net.model_cfg.ROI_HEAD, net.model_cfg.POST_PROCESSING, {k: v.detach().cpu() for k, v in net.state_dict().items()})
    got, it = eng_f32.forward(clouds, return_intermediates=True)
    assert sum(len(g["pred_boxes"]) for g in got) > 10, "nothing survived: the comparison would be vacuous"
    assert it["rois"].shape == bd["rois"].shape
    np.testing.assert_allclose(it["rois"].cpu().numpy(), bd["rois"].cpu().numpy(), atol=1e-4)
    np.testing.assert_array_equal(it["roi_labels"].cpu().numpy(), bd["roi_labels"].cpu().numpy())
    np.testing.assert_allclose(it["batch_box_preds"].cpu().numpy(), bd["batch_box_preds"].cpu().numpy(), atol=2e-4)
    np.testing.assert_allclose(it["batch_cls_preds"].cpu().numpy(), bd["batch_cls_preds"].cpu().numpy(), atol=2e-4)
    # second stage in isolation: the MODULE head (torch Linear / BatchNorm1d stacks, dense voxel2pinds volume) on the engine's own RoIs
    # and levels predicts what the engine's folded GEMMs + index queries predict
    bd2 = dict(batch_size=3, rois=it["rois"], roi_labels=it["roi_labels"], roi_scores=it["roi_scores"], has_class_labels=True,
               multi_scale_3d_features=it["levels"], multi_scale_3d_strides={"x_conv3": 4, "x_conv4": 8})
    with torch.no_grad():
        bd2 = net.roi_head(bd2)
    np.testing.assert_allclose(it["batch_box_preds"].cpu().numpy(), bd2["batch_box_preds"].cpu().numpy(), atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(it["batch_cls_preds"].cpu().numpy(), bd2["batch_cls_preds"].cpu().numpy(), atol=2e-4, rtol=1e-4)
    # post_processing in isolation: the module's per-frame post_processing on the engine's own predictions == the engine's batched one
    bd3 = dict(batch_size=3, batch_box_preds=it["batch_box_preds"], batch_cls_preds=it["batch_cls_preds"], cls_preds_normalized=False,
               has_class_labels=True, roi_labels=it["roi_labels"])
    iso, _ = net.post_processing(bd3)
    for b in range(3):
        _match(got[b], iso[b], 1e-6)
        assert torch.equal(got[b]["pred_boxes"], iso[b]["pred_boxes"]) and torch.equal(got[b]["pred_labels"], iso[b]["pred_labels"])
    # end to end against the module composition: its first stage differs by fp32 rounding (other kernels, other row order), and this
    # random-weight model scores ~20 RoIs that pool nothing within 1e-7 of each other -- their rank, hence which of them the final
    # NMS keeps, is decided by that rounding. Everything else must agree.
    def loose(g, w, atol):
        assert abs(len(g["pred_boxes"]) - len(w["pred_boxes"])) <= 2
        x, y = g["pred_boxes"].cpu().numpy(), w["pred_boxes"].cpu().numpy()
        d = np.abs(x[:, None, :] - y[None, :, :]).max(-1).min(1)
        assert (d <= atol).mean() >= 0.75, float((d <= atol).mean())     # (the near-tied group is ~6 of ~35 boxes)
    for b in range(3):
        loose(got[b], want[b], 1e-3)
    for g, w in zip(eng.forward(clouds), want):           # the default arithmetic (f16x2 first stage)
        loose(g, w, 2e-3)


def test_two_stage_module_in_fast_eval_matches_the_guarded_modules(hip):
    """models.VoxelRCNN through spconv.install(conv_math="f16x2", fast_eval=True) (round 6: the first stage inside the optimistic range
    pass, pair rows between its fused sparse layers; the RoI head reads the pooled levels' `.features`, decoded on demand) against the same
    model on the guarded f16x2 modules: RoIs, second-stage predictions and detections agree to fp32 rounding."""
    from cpd_amd import spconv as sp
    from cpd_amd.spconv.pytorch import conv as spc
    old = (spc.default_conv_math(), spc.fast_eval())
    try:
        sp.install(conv_math="f16x2", fast_eval=False)
        net = _model()
        clouds = _clouds()
        with torch.no_grad():
            want, _, bd = net(_batch_dict(net, clouds))
        sp.install(fast_eval=True)
        with torch.no_grad():
            got, _, bf = net(_batch_dict(net, clouds))
        assert all(t._pairs is not None for t in bf["multi_scale_3d_features"].values())       # the levels did travel as pair rows
        assert sum(len(g["pred_boxes"]) for g in got) > 10
        assert bf["rois"].shape == bd["rois"].shape
        d = (bf["rois"] - bd["rois"]).abs().max(-1)[0]
        assert float((d <= 1e-3).float().mean()) >= 0.9                   # (near-tied proposals may swap ranks between the arithmetics)
        for g, w in zip(got, want):
            assert abs(len(g["pred_boxes"]) - len(w["pred_boxes"])) <= 2
            x, y = g["pred_boxes"].cpu().numpy(), w["pred_boxes"].cpu().numpy()
            dd = np.abs(x[:, None, :] - y[None, :, :]).max(-1).min(1)
            assert (dd <= 2e-3).mean() >= 0.75, float((dd <= 2e-3).mean())
    finally:
        spc.set_default_conv_math(old[0]); spc.set_fast_eval(old[1])


def test_post_processing_matches_a_plain_restatement(hip):
    """detector3d_template.py:222-343 with MULTI_CLASSES_NMS False, has_class_labels True: sigmoid, score threshold, top-k order,
    rotated NMS at 0.3, labels from roi_labels -- restated with torch + the B3 IoU operator, greedy loop on the host."""
    from cpd_amd import iou3d_nms_utils as iu
    net = _model(seed=5)
    g = torch.Generator().manual_seed(2)
    B, R = 2, 120
    boxes = torch.cat([torch.rand(B, R, 2, generator=g) * 30 - 15, torch.rand(B, R, 1, generator=g), torch.rand(B, R, 3, generator=g) * 3 + 1,
                       torch.rand(B, R, 1, generator=g) * 6 - 3], dim=-1).cuda()
    cls = (torch.randn(B, R, 1, generator=g) * 2).cuda()
    cls[:, -7:] = -9.0                                                        # below SCORE_THRESH after the sigmoid
    labels = torch.randint(1, 4, (B, R), generator=g).cuda()
    bd = dict(batch_size=B, batch_box_preds=boxes, batch_cls_preds=cls, cls_preds_normalized=False, has_class_labels=True, roi_labels=labels)
    got, _ = net.post_processing(bd)
    for b in range(B):
        s = torch.sigmoid(cls[b, :, 0])
        idx = torch.nonzero(s >= 0.01).view(-1)
        order = idx[torch.argsort(s[idx], descending=True)]
        iou = iu.boxes_iou_bev(boxes[b][order], boxes[b][order]).cpu().numpy()
        keep, dead = [], np.zeros(len(order), bool)
        for i in range(len(order)):
            if dead[i]:
                continue
            keep.append(i)
            dead |= iou[i] > 0.3
        sel = order[torch.tensor(keep, device=order.device)]
        assert len(got[b]["pred_boxes"]) == len(sel) < R - 7
        torch.testing.assert_close(got[b]["pred_boxes"], boxes[b][sel])
        torch.testing.assert_close(got[b]["pred_scores"], s[sel])
        assert torch.equal(got[b]["pred_labels"], labels[b][sel])


# ---------------------------------------------------------------------------------------------------------------------------------
# Round 5: tight evidence for the BENCHMARKED two-stage path -- full widths, GRID_SIZE 6, the default
# split-fp16 arithmetic, the K = 27 648 stage-split GEMM -- against float64 and against an oracle composition.

def _full_engine(host_results=False):
    from cpd_amd.engine import ModelConfig, init_state_dict
    from cpd_amd.two_stage import VoxelRCNNEngine
    cfg = ModelConfig()
    sd = init_state_dict(cfg, 0)
    mcfg = models.waymo_voxel_rcnn_cfg()
    torch.manual_seed(0)
    head = models.__all__[mcfg.ROI_HEAD.NAME](input_channels={"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 128},
                                              model_cfg=mcfg.ROI_HEAD, point_cloud_range=cfg.point_cloud_range, voxel_size=cfg.voxel_size,
                                              num_class=1)
    with torch.no_grad():
        for m in head.modules():                           # non-trivial BatchNorm statistics; output layers that spread the scores
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.75, 1.25)
                m.weight.uniform_(0.75, 1.25); m.bias.normal_(0, 0.1)
        head.cls_layers[-1].weight.normal_(0, 0.3); head.cls_layers[-1].bias.normal_(0, 0.3)
        head.reg_layers[-1].weight.normal_(0, 0.01); head.reg_layers[-1].bias.zero_()      # residuals of a few per cent: refined boxes stay boxes
    sd.update({"roi_head." + k: v.detach().clone() for k, v in head.state_dict().items()})
    return cfg, mcfg, sd, VoxelRCNNEngine(cfg, mcfg.ROI_HEAD, mcfg.POST_PROCESSING, sd, host_results=host_results)


def test_k_heavy_fc_stacks_f16x2_match_float64(hip):
    """The second stage's FC stacks exactly as `VoxelRCNNEngine` runs them at the bench's size (16 frames x 495 RoIs = 7920 rows):
    27 648 -> 256 (the 8-way stage split of the split-fp16 tile kernel + split_finish), 256 -> 256, and the cls / reg stacks, under
    math = "f16x2" with the range guard's blocks chained -- against float64 GEMMs on the same inputs, <= 1e-4 of O(1) outputs,
    the instantiations asserted through the launch log."""
    cfg, mcfg, sd, eng = _full_engine()
    g = torch.Generator().manual_seed(11)
    n, k = 495 * 16, 27648
    x = torch.relu(torch.randn(n, k, generator=g)).cuda()                  # pooled features are post-ReLU
    fc = eng.head._fc
    with ops.launch_log() as log:
        shared, rb = eng.head._run(fc["shared_fc_layers"], x, math="f16x2", return_block=True)
        cls = eng.head._run(fc["cls_layers"], shared, math="f16x2", in_block=rb)
        reg = eng.head._run(fc["reg_layers"], shared, math="f16x2", in_block=rb)
    names = log.counts
    assert any(nm.startswith("tile_conv_f16s_kernel") for nm in names), names          # the range-guarded split-fp16 tile kernel ...
    assert names.get("split_finish_kernel", 0) >= 1, names                                # ... with its stages dealt to several workgroups
    assert ops.absmax_value(rb) == float(shared.abs().max())                              # the block the last shared layer filled IS max |shared|

    # the float64 stacks straight from the module's own parameters (BatchNorm1d eval formula, not the folded scale / shift)
    def ref_stack(seq, v):
        v = v.double()
        for m in seq:
            if isinstance(m, torch.nn.Linear):
                v = v @ m.weight.double().t()
                if m.bias is not None:
                    v = v + m.bias.double()
            elif isinstance(m, torch.nn.BatchNorm1d):
                v = (v - m.running_mean.double()) / torch.sqrt(m.running_var.double() + m.eps) * m.weight.double() + m.bias.double()
            elif isinstance(m, torch.nn.ReLU):
                v = torch.relu(v)
        return v
    with torch.no_grad():
        want_shared = ref_stack(eng.head.shared_fc_layers, x)
        want_cls = ref_stack(eng.head.cls_layers, want_shared)
        want_reg = ref_stack(eng.head.reg_layers, want_shared)
    for got, want, what in ((shared, want_shared, "shared"), (cls, want_cls, "cls"), (reg, want_reg, "reg")):
        scale = max(1.0, float(want.abs().max()))
        err = float((got.double() - want).abs().max())
        assert err <= 1e-4 * scale, (what, err, scale)
    assert float(want_shared.abs().max()) > 1.0 and float(want_cls.abs().max()) > 0.5        # O(1) outputs: the bound means something
    assert float(want_reg.abs().max()) > 0.01


def test_full_size_two_stage_engine_matches_the_oracle_composition(oracle, hip):
    """`VoxelRCNNEngine` as bench.py's `value_two_stage` runs it -- full widths, GRID_SIZE 6, two radii per level, the default
    split-fp16 arithmetic -- on one full 160k-point frame (last of a batch of two, so that frames with different RoI counts share
    the padded block) against an ORACLE composition: ref_pipeline's first stage, then tests/ref_two_stage.py (oracle.voxel_query,
    numpy grouping + MLPs + FC stacks in float64, oracle.anchor_decode, oracle.nms). RoIs are matched one to one; second-stage
    predictions agree to 1e-3 for every RoI whose neighbour queries took the same decisions in both pipelines -- the RoIs where a
    grid point sits within fp32 rounding of a cell boundary or of the query radius (engine and oracle RoIs differ by ~1e-5) are
    FOUND by running the oracle's queries on the engine's grid points, listed, and bounded; final detections likewise."""
    import ref_pipeline
    import ref_two_stage as r2
    from cpd_amd import roi_pool
    cfg, mcfg, sd, eng = _full_engine()
    pts = waymo_cloud(0)
    ref, rt = ref_pipeline.forward(oracle, cfg, sd, [pts])
    o_rois = ref[0]["pred_boxes"][None].astype(np.float32)
    o_labels = ref[0]["pred_labels"][None]
    n_roi = o_rois.shape[1]
    assert n_roi > 300                                                    # random weights keep ~495 proposals: the bench's load
    clouds = [torch.from_numpy(waymo_cloud(5, n_points=60000)).cuda(), torch.from_numpy(pts).cuda()]
    fi = 1
    got, it = eng.forward(clouds, return_intermediates=True)
    assert torch.isfinite(it["rois"]).all() and torch.isfinite(it["batch_box_preds"]).all()          # padded slots are ZERO boxes
    e_rois = it["rois"][fi].cpu().numpy()
    n_e = int((np.abs(e_rois).sum(-1) > 0).sum())
    assert n_e == n_roi, (n_e, n_roi)
    e_rois = e_rois[:n_roi]
    j = np.abs(e_rois[:, None, :] - o_rois[0][None, :, :]).max(-1).argmin(1)          # engine RoI e <-> oracle RoI j[e]
    assert sorted(j.tolist()) == list(range(n_roi))
    np.testing.assert_allclose(e_rois, o_rois[0][j], atol=1e-3, rtol=1e-4)
    np.testing.assert_array_equal(it["roi_labels"][fi, :n_roi].cpu().numpy(), o_labels[0][j])
    # ---- the oracle's second stage on ITS OWN first stage
    levels = {name: rt["levels"][name] for name in eng.sources}
    final, ot = r2.second_stage(oracle, cfg, mcfg.ROI_HEAD, mcfg.POST_PROCESSING, sd, o_rois, o_labels, levels, 1)
    # ---- which RoIs' neighbour queries decide differently on the engine's grid points (same device function the engine calls)
    e_grid, _ = roi_pool.roi_grid_points(it["rois"][fi:fi + 1, :n_roi].contiguous(), eng.head.grid_size, cfg.voxel_size, cfg.point_cloud_range)
    e_grid = e_grid.view(n_roi, -1, 3).cpu().numpy()                                   # (n_roi, 216, 3), engine RoI order
    inv = np.empty(n_roi, np.int64); inv[j] = np.arange(n_roi)                        # oracle RoI o <-> engine RoI inv[o]
    o_grid, _ = r2.grid_points(o_rois, eng.head.grid_size)
    assert float(np.abs(e_grid[inv] - o_grid).max()) <= 2e-3                          # the same grid up to the RoIs' rounding
    strides = {"x_conv3": 4, "x_conv4": 8}
    _, q_e = r2.roi_grid_pool(oracle, sd, mcfg.ROI_HEAD, o_rois, levels, strides, cfg.voxel_size, cfg.point_cloud_range, 1, grid_xyz=e_grid[inv])
    g3 = eng.head.grid_size ** 3
    flip = np.zeros(n_roi, bool)
    for key, (idx_o, empty_o) in ot["queries"].items():
        idx_e, empty_e = q_e[key]
        d = (idx_o != idx_e).any(1) | (empty_o != empty_e)
        flip |= d.reshape(n_roi, g3).any(1)
    flips = np.nonzero(flip)[0]
    print("RoIs whose neighbour queries decide differently on the engine's grid points (oracle order):", flips.tolist())
    assert len(flips) <= max(3, int(0.04 * n_roi)), len(flips)
    # ---- second-stage predictions, RoI by RoI
    e_cls = it["batch_cls_preds"][fi, :n_roi].cpu().numpy()[inv]
    e_box = it["batch_box_preds"][fi, :n_roi].cpu().numpy()[inv]
    o_cls, o_box = ot["batch_cls_preds"][0], ot["batch_box_preds"][0]
    same = ~flip
    assert same.sum() >= 0.96 * n_roi
    np.testing.assert_allclose(e_cls[same], o_cls[same], atol=1e-3, rtol=0)
    np.testing.assert_allclose(e_box[same], o_box[same], atol=1e-3, rtol=1e-4)
    assert float(np.abs(e_cls - o_cls).max()) < 0.5                                   # ... and a flipped RoI moves a little, not wildly
    # ---- final detections. post_processing is a greedy NMS in score order: two RoIs whose scores differ by less than the 1e-3 the
    # predictions are compared at may swap ranks between the pipelines, and one swapped suppression decision cascades through the
    # frame's ~470 kept boxes -- so the stage is checked where it is DEFINED: the oracle's post_processing (fp32 sigmoid, stable
    # descending order, oracle.nms at 0.3) on the ENGINE's own second-stage predictions must select exactly the engine's detections.
    # (the whole padded block: like the reference, the engine refines and post-processes the zero RoIs that pad a frame up to the
    # batch's largest proposal count -- roi_head_template.py:53-114 / detector3d_template.py:222-343 make no exception for them)
    e_cls_f = it["batch_cls_preds"][fi:fi + 1].cpu().numpy()
    e_box_f = it["batch_box_preds"][fi:fi + 1].cpu().numpy()
    e_lab_f = it["roi_labels"][fi:fi + 1].cpu().numpy()
    n_pad = e_cls_f.shape[1] - n_roi
    pp = r2.post_processing(oracle, mcfg.POST_PROCESSING, e_box_f, e_cls_f, e_lab_f, sigmoid_dtype=np.float32)[0]
    a = got[fi]["pred_boxes"].cpu().numpy()
    assert len(a) > 10 and len(a) == len(pp["pred_boxes"]), (len(a), len(pp["pred_boxes"]))
    np.testing.assert_array_equal(a, pp["pred_boxes"])
    np.testing.assert_allclose(got[fi]["pred_scores"].cpu().numpy(), pp["pred_scores"], atol=1e-6)
    np.testing.assert_array_equal(got[fi]["pred_labels"].cpu().numpy(), pp["pred_labels"])
    # the production call (no intermediates): the pooled levels reach the second stage as fp16-pair rows (split-fp16 first GEMM of the
    # pooling instead of the fp32 wave kernel on decoded rows) -- the same detections up to fp32 rounding
    got_p = eng.forward(clouds)
    ap = got_p[fi]["pred_boxes"].cpu().numpy()
    dp = np.abs(ap[:, None, :] - a[None, :, :]).max(-1)
    assert abs(len(ap) - len(a)) <= 3 and (dp.min(1) <= 1e-3).mean() >= 0.97, (len(ap), len(a), float((dp.min(1) <= 1e-3).mean()))
    # end to end (informational + a floor): detections of the oracle's own chain that the engine also reports, at 1e-3
    b = final[0]["pred_boxes"]
    d = np.abs(a[:, None, :] - b[None, :, :]).max(-1)
    common = int((d.min(1) <= 1e-3).sum())
    print("final detections: engine %d, oracle chain %d, in common at 1e-3: %d (rank swaps among scores closer than 1e-3 cascade through "
          "the greedy NMS; %d RoIs with flipped neighbour queries)" % (len(a), len(b), common, len(flips)))
    assert abs(len(a) - n_pad - len(b)) <= 0.1 * len(b) and common >= 0.6 * len(b)


# ---------------------------------------------------------------------------------------------------------------------------------
# The OTHER shipped two-stage family (voxel_rcnn_dbscan / oyster_single_train.yaml: AnchorHeadSingleV2 proposals -> VoxelRCNNHead):
# cpd_amd.anchor_engine.AnchorPointEngine as the fused engine's first stage.

def _anchor_model(seed=7):
    cfg = models.waymo_voxel_rcnn_dbscan_cfg()
    cfg.BACKBONE_2D.NUM_FILTERS, cfg.BACKBONE_2D.NUM_UPSAMPLE_FILTERS, cfg.BACKBONE_2D.LAYER_NUMS = [64, 128], [128, 128], [2, 2]
    torch.manual_seed(seed)
    net = models.VoxelRCNN(cfg, point_cloud_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 4.0]).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.75, 1.25)
                m.weight.uniform_(0.75, 1.25); m.bias.normal_(0, 0.1)
        for br in net.dense_head.BRANCHES:                                       # the reference's N(0, 0.001) branch convs leave every anchor at its bias:
            getattr(net.dense_head, br)[0].weight.normal_(0, (2.0 / (9 * 64)) ** 0.5)   # spread the features ...
        net.dense_head.conv_cls[3].weight.normal_(0, 0.5)                       # ... and the anchor scores
        net.dense_head.conv_reg[3].weight.normal_(0, 0.02); net.dense_head.conv_dim[3].weight.normal_(0, 0.02)
        net.roi_head.cls_layers[-1].weight.normal_(0, 0.3); net.roi_head.cls_layers[-1].bias.normal_(0, 0.3)
        net.roi_head.reg_layers[-1].weight.normal_(0, 0.01); net.roi_head.reg_layers[-1].bias.zero_()
    return net


def test_anchor_two_stage_engine_matches_the_module_composition(hip):
    from cpd_amd import spconv as sp
    sp.install(conv_math="f32")
    net = _anchor_model()
    net.dense_head.conv_math = "f32"
    clouds = _clouds()
    bd = _batch_dict(net, clouds)
    bd["points"] = torch.cat([torch.nn.functional.pad(c, (1, 0), value=float(b)) for b, c in enumerate(clouds)])
    with torch.no_grad():
        for m in net.module_list[:-1]:
            bd = m(bd)
        dense = dict(cls=bd["batch_cls_preds"].clone(), box=bd["batch_box_preds"].clone())
        bd = net.roi_head(bd)
        want, _ = net.post_processing(bd)
    assert bd["rois"].shape[1] == 200
    ecfg = net.to_engine_config()
    ecfg.conv_math = "f32"
    from cpd_amd.anchor_engine import AnchorPointEngine
    from cpd_amd.two_stage import VoxelRCNNEngine
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    rpn = AnchorPointEngine(ecfg, sd, net.model_cfg.DENSE_HEAD, net.model_cfg.ROI_HEAD.NMS_CONFIG["TEST"])
    eng = VoxelRCNNEngine(ecfg, net.model_cfg.ROI_HEAD, net.model_cfg.POST_PROCESSING, sd, rpn=rpn)
    got, it = eng.forward(clouds, return_intermediates=True)
    assert sum(len(g["pred_boxes"]) for g in got) > 10, "nothing survived: the comparison would be vacuous"
    # first stage: the anchor head's decoded predictions, anchor for anchor (same occupancy mask, same anchor order)
    np.testing.assert_allclose(rpn.last_dense["batch_cls_preds"].cpu().numpy(), dense["cls"].cpu().numpy(), atol=2e-4)
    np.testing.assert_allclose(rpn.last_dense["batch_box_preds"].cpu().numpy(), dense["box"].cpu().numpy(), atol=2e-4, rtol=1e-4)
    # proposals: 200 per frame out of ~15000 anchors ranked by a score; anchors whose scores differ by less than the two pipelines'
    # rounding may swap ranks, so the RoI sets are matched by geometry
    assert it["rois"].shape == bd["rois"].shape
    for b in range(3):
        x, y = it["rois"][b].cpu().numpy(), bd["rois"][b].cpu().numpy()
        d = np.abs(x[:, None, :] - y[None, :, :]).max(-1)
        assert (d.min(1) <= 1e-3).mean() >= 0.95, float((d.min(1) <= 1e-3).mean())
    # second stage in isolation: the MODULE head on the engine's own RoIs and levels predicts what the engine predicts
    bd2 = dict(batch_size=3, rois=it["rois"], roi_labels=it["roi_labels"], roi_scores=it["roi_scores"], has_class_labels=True,
               multi_scale_3d_features=it["levels"], multi_scale_3d_strides={"x_conv3": 4, "x_conv4": 8})
    with torch.no_grad():
        bd2 = net.roi_head(bd2)
    np.testing.assert_allclose(it["batch_box_preds"].cpu().numpy(), bd2["batch_box_preds"].cpu().numpy(), atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(it["batch_cls_preds"].cpu().numpy(), bd2["batch_cls_preds"].cpu().numpy(), atol=2e-4, rtol=1e-4)
    # post_processing in isolation: exact
    bd3 = dict(batch_size=3, batch_box_preds=it["batch_box_preds"], batch_cls_preds=it["batch_cls_preds"], cls_preds_normalized=False,
               has_class_labels=True, roi_labels=it["roi_labels"])
    iso, _ = net.post_processing(bd3)
    for b in range(3):
        assert torch.equal(got[b]["pred_boxes"], iso[b]["pred_boxes"]) and torch.equal(got[b]["pred_labels"], iso[b]["pred_labels"])
    # end to end: most detections in common
    for g, w in zip(got, want):
        x, y = g["pred_boxes"].cpu().numpy(), w["pred_boxes"].cpu().numpy()
        assert abs(len(x) - len(y)) <= max(3, 0.1 * len(y))
        if len(x) and len(y):
            d = np.abs(x[:, None, :] - y[None, :, :]).max(-1).min(1)
            assert (d <= 2e-3).mean() >= 0.8, float((d <= 2e-3).mean())
    # the proposal NMS looks at each frame's first max(512, 4 x NMS_POST_MAXSIZE) candidates (cpd_nms_batch_first); 64 candidates cannot hold
    # 200 survivors, so the `incomplete` word sends the step through the full NMS -- and all of the anchors is the full NMS itself: the
    # same RoIs bit for bit, three ways
    base = (it["rois"].clone(), it["roi_scores"].clone(), it["roi_labels"].clone())
    for rows, reruns in ((64, 1), (1 << 20, 0)):
        rpn.proposal_first_rows, rpn.proposal_full_reruns = rows, 0
        _, it_r = eng.forward(clouds, return_intermediates=True)
        assert rpn.proposal_full_reruns == reruns, (rows, rpn.proposal_full_reruns)
        assert torch.equal(it_r["rois"], base[0]) and torch.equal(it_r["roi_scores"], base[1]) and torch.equal(it_r["roi_labels"], base[2])
    rpn.proposal_first_rows = None
    # ... and through the model's own to_engine() in the default arithmetic
    eng2 = net.to_engine()
    assert type(eng2.rpn).__name__ == "AnchorPointEngine"
    got2 = eng2.forward(clouds)
    assert all(torch.isfinite(g["pred_boxes"]).all() for g in got2) and sum(len(g["pred_boxes"]) for g in got2) > 10


def test_anchor_engine_reruns_an_out_of_range_step_guarded_and_stays_guarded(hip):
    """The f16x2 range guard through AnchorPointEngine's own decode_and_nms (its verdict rides behind the proposal NMS's `incomplete`
    word): a backbone running 3e4 times hotter, past 2^15, is flagged by the optimistic pass and re-run guarded, once, with a warning;
    the next step starts guarded -- no second pass -- and gives the same proposals bit for bit. (conv_out's BatchNorm brings the dense half
    back to ordinary magnitudes, as in test_gpu_head_at_peaks.py::test_range_guard_rerun_matches.)"""
    from cpd_amd.anchor_engine import AnchorPointEngine
    net = _anchor_model()
    clouds = _clouds()
    ecfg = net.to_engine_config()
    ecfg.conv_math = "f16x2"
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    sd["backbone_3d.conv_input.1.weight"] = sd["backbone_3d.conv_input.1.weight"] * 3e4
    sd["backbone_3d.conv_input.1.bias"] = sd["backbone_3d.conv_input.1.bias"] * 3e4
    sd["backbone_3d.conv_out.1.weight"] = sd["backbone_3d.conv_out.1.weight"] / 3e4
    rpn = AnchorPointEngine(ecfg, sd, net.model_cfg.DENSE_HEAD, net.model_cfg.ROI_HEAD.NMS_CONFIG["TEST"])
    with pytest.warns(UserWarning, match="range-guarded"):
        first = rpn.forward(clouds, proposals=["x_conv3", "x_conv4"])[:4]
    assert (rpn.range_reruns, rpn.range_guarded_steps) == (1, 1)
    again = rpn.forward(clouds, proposals=["x_conv3", "x_conv4"])[:4]
    assert (rpn.range_reruns, rpn.range_guarded_steps) == (1, 2)
    assert len(first[3]) == 3 and min(first[3]) > 0 and again[3] == first[3]
    for a, b in zip(first[:3], again[:3]):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def _full_anchor_engine():
    """the model of bench.py's `value_two_stage_anchor`, from the same builder (cpd_amd.anchor_engine.synthetic_two_stage_state)"""
    from cpd_amd.anchor_engine import AnchorPointEngine, synthetic_two_stage_state
    from cpd_amd.engine import ModelConfig, init_state_dict
    from cpd_amd.two_stage import VoxelRCNNEngine
    cfg = ModelConfig()
    mcfg, sd = synthetic_two_stage_state(cfg, init_state_dict(cfg, 0), seed=1)
    rpn = AnchorPointEngine(cfg, sd, mcfg.DENSE_HEAD, mcfg.ROI_HEAD.NMS_CONFIG["TEST"])
    return cfg, mcfg, sd, rpn, VoxelRCNNEngine(cfg, mcfg.ROI_HEAD, mcfg.POST_PROCESSING, sd, rpn=rpn)


def test_full_size_anchor_two_stage_engine_matches_the_oracle_composition(oracle, hip):
    """`AnchorPointEngine` -> `VoxelRCNNEngine` exactly as bench.py's `value_two_stage_anchor` runs them (full widths,
    174 600 anchors on the full BEV map, the default split-fp16 arithmetic, GRID_SIZE 6) on one full 160k-point frame -- the last of a batch
    of two, so that the occupancy mask is a batch's and the RoI block is padded -- against an ORACLE composition:
    tests/ref_pipeline.py (voxelizer ... BaseBEVBackbone), tests/ref_anchor.py (AnchorHeadSingleV2 unfused, oracle.anchor_decode,
    proposal_layer on oracle.nms; anchor_head_single.py:31-192, roi_head_template.py:53-114) and tests/ref_two_stage.second_stage.
    Dense predictions anchor for anchor; proposals matched one to one by geometry at 1e-3 (rank swaps among scores closer than the
    arithmetics' rounding are LISTED); second-stage predictions RoI by RoI for every RoI whose neighbour queries decide the same on both
    pipelines' grid points; final detections where the stage is defined. Then the proposal NMS's fallbacks at full size."""
    import ref_anchor as ra
    import ref_two_stage as r2
    from cpd_amd import anchor_head, roi_pool
    cfg, mcfg, sd, rpn, eng = _full_anchor_engine()
    assert cfg.conv_math == "f16x2"
    pts = waymo_cloud(0)
    other = waymo_cloud(5, n_points=60000)
    clouds = [torch.from_numpy(other).cuda(), torch.from_numpy(pts).cuda()]
    fi = 1
    got, it = eng.forward(clouds, return_intermediates=True)
    assert getattr(rpn, "proposal_full_reruns", 0) == 0                  # the first 800 candidates held the 200 survivors: the fast path ran
    # ---- the oracle's first stage (anchors: the generator on the CPU, pinned on the reference class's golden in test_anchor_head.py)
    grid = oracle.grid_size(cfg.voxel_size, cfg.point_cloud_range)[::-1]
    agc = mcfg.DENSE_HEAD["ANCHOR_GENERATOR_CONFIG"]
    fms = [[grid[0] // c["feature_map_stride"], grid[1] // c["feature_map_stride"]] for c in agc]
    anchors_root = [a.numpy() for a in anchor_head.AnchorGenerator(cfg.point_cloud_range, agc).generate_anchors(fms, device="cpu")[0]]
    nms_cfg = mcfg.ROI_HEAD.NMS_CONFIG["TEST"]
    fs = ra.first_stage(oracle, cfg, mcfg.DENSE_HEAD, nms_cfg, sd, pts, anchors_root, mask_points_xy=np.concatenate([other[:, :2], pts[:, :2]]))
    # ---- dense head: same occupancy mask, same anchors, predictions anchor for anchor
    np.testing.assert_array_equal(rpn.last_dense["anchor_mask"].cpu().numpy(), fs["mask"])
    e_cls = rpn.last_dense["batch_cls_preds"][fi].cpu().numpy()
    e_box = rpn.last_dense["batch_box_preds"][fi].cpu().numpy()
    assert e_cls.shape == fs["batch_cls_preds"][0].shape and e_cls.shape[0] > 150000
    scale = max(1.0, float(np.abs(fs["batch_cls_preds"]).max()))         # the spread class scores reach +-13: 1e-4 of the outputs' scale
    np.testing.assert_allclose(e_cls, fs["batch_cls_preds"][0], atol=1e-4 * scale, rtol=0)
    np.testing.assert_allclose(e_box, fs["batch_box_preds"][0], atol=1e-3, rtol=1e-4)          # (decoded: exp() of the size residuals, metres)
    # ---- proposals: 200 of 174 600 anchors, ranked by a score both pipelines know to ~1e-5
    n_roi = int(fs["kept"][0])
    assert n_roi == int(nms_cfg["NMS_POST_MAXSIZE"]) == 200
    e_rois = it["rois"][fi].cpu().numpy()
    assert e_rois.shape[0] == n_roi and int((np.abs(e_rois).sum(-1) > 0).sum()) == n_roi
    o_rois = fs["rois"]
    d = np.abs(e_rois[:, None, :] - o_rois[0][None, :, :]).max(-1)
    j = d.argmin(1)                                                       # engine RoI e <-> oracle RoI j[e]
    hit = d[np.arange(n_roi), j] <= 1e-3
    lost = np.nonzero(~hit)[0]
    print("engine RoIs without an oracle partner at 1e-3 (rank swaps at the NMS_PRE_MAXSIZE cut or among near-equal scores):", lost.tolist())
    assert hit.mean() >= 0.97 and len(set(j[hit].tolist())) == int(hit.sum())        # one to one
    np.testing.assert_allclose(e_rois[hit], o_rois[0][j[hit]], atol=1e-3, rtol=1e-4)
    np.testing.assert_array_equal(it["roi_labels"][fi].cpu().numpy()[hit], fs["roi_labels"][0][j[hit]])
    np.testing.assert_allclose(it["roi_scores"][fi].cpu().numpy()[hit], fs["roi_scores"][0][j[hit]], atol=1e-4 * scale)
    assert np.abs(j[hit] - np.nonzero(hit)[0]).max() <= 3 + len(lost)     # ... and only neighbours in the ranking swap
    # ---- the oracle's second stage on ITS OWN first stage
    levels = {name: fs["levels"][name] for name in eng.sources}
    final, ot = r2.second_stage(oracle, cfg, mcfg.ROI_HEAD, mcfg.POST_PROCESSING, sd, o_rois, fs["roi_labels"], levels, 1)
    # RoIs whose neighbour queries decide differently on the engine's grid points (same recipe as the CenterPoint engine's test above)
    e_grid, _ = roi_pool.roi_grid_points(it["rois"][fi:fi + 1].contiguous(), eng.head.grid_size, cfg.voxel_size, cfg.point_cloud_range)
    e_grid = e_grid.view(n_roi, -1, 3).cpu().numpy()
    o_grid, _ = r2.grid_points(o_rois, eng.head.grid_size)
    eo = np.nonzero(hit)[0]                                               # engine RoIs with a partner, and their oracle RoIs
    oo = j[hit]
    assert float(np.abs(e_grid[eo] - o_grid[oo]).max()) <= 2e-3
    grid_for_oracle = o_grid.copy()
    grid_for_oracle[oo] = e_grid[eo]
    strides = {"x_conv3": 4, "x_conv4": 8}
    _, q_e = r2.roi_grid_pool(oracle, sd, mcfg.ROI_HEAD, o_rois, levels, strides, cfg.voxel_size, cfg.point_cloud_range, 1, grid_xyz=grid_for_oracle)
    g3 = eng.head.grid_size ** 3
    flip = np.zeros(n_roi, bool)
    for key, (idx_o, empty_o) in ot["queries"].items():
        idx_e, empty_e = q_e[key]
        dd = (idx_o != idx_e).any(1) | (empty_o != empty_e)
        flip |= dd.reshape(n_roi, g3).any(1)
    print("RoIs whose neighbour queries decide differently on the engine's grid points (oracle order):", np.nonzero(flip)[0].tolist())
    assert flip.sum() <= max(3, int(0.05 * n_roi)), int(flip.sum())
    same = ~flip[oo]
    e_cls2 = it["batch_cls_preds"][fi].cpu().numpy()[eo][same]
    e_box2 = it["batch_box_preds"][fi].cpu().numpy()[eo][same]
    assert same.sum() >= 0.92 * n_roi
    np.testing.assert_allclose(e_cls2, ot["batch_cls_preds"][0][oo][same], atol=1e-3, rtol=0)
    np.testing.assert_allclose(e_box2, ot["batch_box_preds"][0][oo][same], atol=1e-3, rtol=1e-4)
    # ---- final detections where the stage is DEFINED: the oracle's post_processing on the ENGINE's own second-stage predictions (the
    # whole padded block; padded slots carry label 1 like the reference's proposal_layer, roi_head_template.py:111)
    e_cls_f = it["batch_cls_preds"][fi:fi + 1].cpu().numpy()
    e_box_f = it["batch_box_preds"][fi:fi + 1].cpu().numpy()
    e_lab_f = it["roi_labels"][fi:fi + 1].cpu().numpy()
    pp = r2.post_processing(oracle, mcfg.POST_PROCESSING, e_box_f, e_cls_f, e_lab_f, sigmoid_dtype=np.float32)[0]
    a = got[fi]["pred_boxes"].cpu().numpy()
    assert len(a) > 10 and len(a) == len(pp["pred_boxes"]), (len(a), len(pp["pred_boxes"]))
    np.testing.assert_array_equal(a, pp["pred_boxes"])
    np.testing.assert_allclose(got[fi]["pred_scores"].cpu().numpy(), pp["pred_scores"], atol=1e-6)
    np.testing.assert_array_equal(got[fi]["pred_labels"].cpu().numpy(), pp["pred_labels"])
    # the shorter frame of the batch found its 200 proposals too; had it found fewer, its padded slots would be zero boxes of label 1
    assert it["roi_labels"].min() >= 1
    # end to end (informational + a floor)
    b = final[0]["pred_boxes"]
    dd = np.abs(a[:, None, :] - b[None, :, :]).max(-1)
    common = int((dd.min(1) <= 1e-3).sum())
    print("final detections: engine %d, oracle chain %d, in common at 1e-3: %d" % (len(a), len(b), common))
    assert abs(len(a) - len(b)) <= 0.1 * len(b) and common >= 0.6 * len(b)
    # the production call (pair-row levels into the pooling's first GEMM): the same detections up to fp32 rounding
    ap = eng.forward(clouds)[fi]["pred_boxes"].cpu().numpy()
    dp = np.abs(ap[:, None, :] - a[None, :, :]).max(-1)
    assert abs(len(ap) - len(a)) <= 3 and (dp.min(1) <= 1e-3).mean() >= 0.97
    # ---- the proposal NMS's two fallbacks on this full frame. (i) 64 first rows cannot hold 200 survivors: the `incomplete` word sends
    # the step through the full 4096-candidate NMS (cpd_nms_batch) -- the same RoIs bit for bit; all rows: the full NMS itself
    base = (it["rois"].clone(), it["roi_scores"].clone(), it["roi_labels"].clone())
    for rows, reruns in ((64, 1), (1 << 20, 0)):
        rpn.proposal_first_rows, rpn.proposal_full_reruns = rows, 0
        _, it_r = eng.forward(clouds, return_intermediates=True)
        assert rpn.proposal_full_reruns == reruns, (rows, rpn.proposal_full_reruns)
        assert torch.equal(it_r["rois"], base[0]) and torch.equal(it_r["roi_scores"], base[1]) and torch.equal(it_r["roi_labels"], base[2])
    rpn.proposal_first_rows = None
    # (ii) the device fallback of the module path (cpd_nms_batch_first + cpd_nms_batch_where, no read-back) on the engine's dense
    # predictions: frames that need more than their first 64 / 256 rows are finished on the device -- the full call's answer, exactly
    cls_d, box_d = rpn.last_dense["batch_cls_preds"], rpn.last_dense["batch_box_preds"]
    args = (box_d, cls_d, float(nms_cfg["NMS_THRESH"]), int(nms_cfg["NMS_PRE_MAXSIZE"]), int(nms_cfg["NMS_POST_MAXSIZE"]))
    full = roi_pool.proposal_layer(*args)
    assert torch.equal(full[0], base[0]) and torch.equal(full[2], base[2])
    for rows in (64, 256, "auto"):
        dev = roi_pool.proposal_layer(*args, first_rows=rows, device_fallback=True)
        for x, y in zip(dev, full):
            assert torch.equal(x, y), rows
    inc = roi_pool.proposal_layer(*args, first_rows=64)[4]
    assert int(inc.min()) == 1                                            # (every frame DID need the fallback at 64 rows)


def test_rank_scores_kernel_matches_the_torch_sequence(hip):
    """cpd_rank_scores against the torch sequence of post_processing it replaces (sigmoid, max over classes, threshold, stable descending
    sort, gathers), incl. ties (lower index first), rows below the threshold, NaN logits and the pre-NMS cap."""
    g = torch.Generator().manual_seed(9)
    B, R, C = 3, 497, 3
    cls = (torch.randn(B, R, C, generator=g) * 2).cuda()
    cls[0, 10] = cls[0, 3]                                   # an exact tie
    cls[1, 7, :] = float("nan")
    cls[2, :50] = -9.0                                       # below the threshold after the sigmoid
    boxes = torch.randn(B, R, 7, generator=g).cuda()
    labels = torch.randint(1, 4, (B, R), generator=g).cuda()
    thr, pre = 0.3, 400
    ob, osc, ol, n_ok = ops.rank_scores(cls, boxes, labels, thr, pre)
    scores = torch.sigmoid(cls).max(dim=-1)[0]
    ok = scores >= thr
    ranked, order = torch.sort(torch.where(ok, scores, torch.full_like(scores, -1.0)), dim=1, descending=True, stable=True)
    assert n_ok.tolist() == ok.sum(dim=1).clamp(max=pre).tolist()
    np.testing.assert_allclose(osc.cpu().numpy(), ranked.cpu().numpy(), atol=1e-6, rtol=0)
    for b in range(B):
        k = int(ok[b].sum())
        # (rows the two sigmoids round to scores one ulp apart may swap with a neighbour: compare the ranked prefix as a set first)
        assert set(map(tuple, ob[b, :k].cpu().numpy().round(5).tolist())) == set(map(tuple, boxes[b][order[b, :k]].cpu().numpy().round(5).tolist()))
        same = (ob[b, :k] == boxes[b][order[b, :k]]).all(dim=1)
        assert float(same.float().mean()) >= 0.99
        assert torch.equal(ol[b, :k][same].long(), labels[b][order[b, :k]][same])
    i3, i10 = [int((ob[0] == boxes[0, i]).all(dim=1).nonzero()[0]) for i in (3, 10)]
    assert i10 == i3 + 1                                     # the tie: lower index first
