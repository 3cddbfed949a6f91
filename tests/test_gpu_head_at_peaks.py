"""The engines with CenterHead's regression branches evaluated at the peaks only (ModelConfig.head_at_peaks) against the same engines
on the full head maps, from the same state dict.

The rule, everywhere: per frame the number of detections, the labels and the scores are IDENTICAL (the hm branch runs the same kernel
on the same tile either way; engine._head_at_peaks_ok), boxes within 1e-4 absolute. The decode's outputs before the NMS are compared
as well; a box moved by 1e-6 can change an NMS decision only at an exact tie, so where the kept sets differ the test looks up the pair
that decided and fails unless its IoU is within 1e-5 of nms_thresh.
"""
import dataclasses
import warnings

import numpy as np
import pytest
import torch

from cpd_amd import models, ops
from cpd_amd.engine import CenterPointEngine, ModelConfig, init_state_dict
from cpd_amd.synthetic import waymo_cloud

pytestmark = pytest.mark.gpu

BOX_ATOL = 1e-4


def small_cfg():
    return ModelConfig(point_cloud_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 4.0], post_center_limit_range=[-20, -20, -2, 20, 20, 4],
                       bev_num_filters=[64, 128], bev_num_upsample_filters=[128, 128], bev_layer_nums=[1, 1], max_obj_per_sample=100)


def small_clouds(n=2):
    out = []
    for s in range(n):
        p = waymo_cloud(s, n_points=40000)
        p[:, :2] *= 0.3
        out.append(torch.from_numpy(p).cuda())
    return out


def full_clouds(n):
    return [torch.from_numpy(waymo_cloud(s, n_points=60000 + 20000 * s)).cuda() for s in range(n)]


def pair(cfg, sd, cls=CenterPointEngine, **kw):
    """(engine at the peaks, engine on the full maps) from one state dict"""
    return tuple(cls(dataclasses.replace(cfg, head_at_peaks=on, head_at_peaks_min_frames=1), sd, **kw) for on in (True, False))


class Tap:
    """records what the decode handed to the NMS (ops.nms_batch: boxes, counts) and what the NMS kept (ops.select_boxes)"""

    def __init__(self, monkeypatch):
        self.nms, self.sel = [], []
        real_nms, real_sel = ops.nms_batch, ops.select_boxes

        def nms_spy(boxes, counts, *a, **k):
            self.nms.append((boxes.clone(), counts.clone()))
            return real_nms(boxes, counts, *a, **k)

        def sel_spy(boxes, scores, labels, keep, num_keep, *a, **k):
            self.sel.append((scores.clone(), labels.clone(), keep.clone(), num_keep.clone()))
            return real_sel(boxes, scores, labels, keep, num_keep, *a, **k)
        monkeypatch.setattr(ops, "nms_batch", nms_spy)
        monkeypatch.setattr(ops, "select_boxes", sel_spy)

    def pop(self):
        """(boxes, counts, scores, labels, keep, num_keep) of the last step (a re-run step's last pass)"""
        out = self.nms[-1] + self.sel[-1]
        self.nms, self.sel = [], []
        return out


def assert_same_decode(on, off, nms_thresh):
    """pre-NMS: the decode's compacted outputs; then the kept sets (see the module docstring)"""
    (b1, c1, s1, l1, k1, n1), (b0, c0, s0, l0, k0, n0) = on, off
    assert torch.equal(c1, c0)
    for f, n in enumerate(c0.tolist()):
        assert torch.equal(s1[f, :n], s0[f, :n]) and torch.equal(l1[f, :n], l0[f, :n])
        if n:
            err = (b1[f, :n] - b0[f, :n]).abs()
            err[:, 6] = torch.minimum(err[:, 6], 2 * np.pi - err[:, 6])
            assert float(err.max()) <= BOX_ATOL
        a, b = k1[f, :int(n1[f])].tolist(), k0[f, :int(n0[f])].tolist()
        if a == b:
            continue
        # the first candidate one run kept and the other suppressed: an earlier kept box of the run that suppressed it decided
        i = min(set(a) ^ set(b))
        boxes, kept = (b0, b) if i in a else (b1, a)
        earlier = [j for j in kept if j < i]
        assert earlier, "frame %d: candidate %d dropped with no earlier box to suppress it" % (f, i)
        iou = ops.boxes_iou_bev(boxes[f, earlier].contiguous(), boxes[f, i:i + 1].contiguous()).view(-1)
        gap = float((iou - nms_thresh).abs().min())
        assert gap <= 1e-5, "frame %d: candidate %d kept by one path only; the nearest IoU is %g from the threshold" % (f, i, gap)
        pytest.fail("frame %d: an NMS tie at candidate %d (IoU within 1e-5 of the threshold): the kept sets differ" % (f, i))


def _box_err(a, b):
    """|a - b| of [..., 7] boxes, the heading's difference taken on the circle"""
    err = (a - b).abs()
    err[..., 6] = torch.minimum(err[..., 6], 2 * np.pi - err[..., 6])
    return err


def assert_same_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["pred_boxes"].shape == w["pred_boxes"].shape
        assert torch.equal(g["pred_labels"].cpu(), w["pred_labels"].cpu()) and torch.equal(g["pred_scores"].cpu(), w["pred_scores"].cpu())
        if len(g["pred_boxes"]):
            err = (g["pred_boxes"].cpu() - w["pred_boxes"].cpu()).abs()
            err[:, 6] = torch.minimum(err[:, 6], 2 * np.pi - err[:, 6])
            assert float(err.max()) <= BOX_ATOL


def compare(engines, clouds, tap, active):
    on, off = engines
    for host in (False, True):
        on.host_results = off.host_results = host
        r1 = on.forward(clouds)
        assert on.last_head_at_peaks == active
        d1 = tap.pop()
        r0 = off.forward(clouds)
        assert not off.last_head_at_peaks
        d0 = tap.pop()
        assert all(r["pred_boxes"].is_cuda != host for r in r1)
        assert sum(len(r["pred_boxes"]) for r in r0) > 10, "nothing detected: the comparison would be vacuous"
        assert_same_results(r1, r0)
        assert_same_decode(d1, d0, on.cfg.nms_thresh)
    on.host_results = off.host_results = False


@pytest.fixture()
def tap(monkeypatch):
    return Tap(monkeypatch)


@pytest.fixture(scope="module")
def full(hip):
    cfg = ModelConfig()
    sd = init_state_dict(cfg, 0)
    on, off = pair(cfg, sd)
    _, h, w = on._final_shape()
    batch = next(b for b in range(1, 9) if on.dense_pairs_ok(b, h, w))
    return cfg, sd, on, off, batch, full_clouds(batch)


def test_reduced_config_two_frames_fp32_maps(hip, tap):
    """+-20 m, two frames: fp32 dense maps. At 50 x 50 pixels the 64-column layers take no window tile, so the step keeps the full maps
    (engine._head_at_peaks_ok): the fall-back is what runs here, and it is today's path bit for bit."""
    cfg = small_cfg()
    engines = pair(cfg, init_state_dict(cfg, seed=1))
    _, h, w = engines[0]._final_shape()
    assert not engines[0].dense_pairs_ok(2, h, w)
    compare(engines, small_clouds(2), tap, active=engines[0]._head_at_peaks_ok(2, h, w))


def test_full_size_pair_maps(full, tap):
    cfg, sd, on, off, batch, clouds = full
    _, h, w = on._final_shape()
    assert on._head_at_peaks_ok(batch, h, w)
    with ops.launch_log() as log1:
        on.forward(clouds)
    with ops.launch_log() as log0:
        off.forward(clouds)
    tap.pop()
    assert on.last_head_at_peaks and on.range_reruns == 0
    # what the conv launch log carries of the new path (its keys are kernel instantiations: tiles, not channel counts): the window
    # launches are the same three kernels the same number of times (head1_hm and head2_hm take head1's and head2's tiles: the gate), and
    # the regression branches' first convs are ONE added row-wave launch on pair rows that writes fp32 rows -- the only launch of that kind
    window = lambda log: {k: v for k, v in log.counts.items() if k.startswith("window_conv")}
    assert window(log1) == window(log0) and any(k.startswith("window_conv_f16p_kernel<16,") for k in log1.counts), (log1.counts, log0.counts)
    fp32_out = lambda log: sum(v for k, v in log.counts.items() if k.startswith(("rowwave_conv_f16p_kernel", "rowwave_conv_f16pw_kernel")))
    assert fp32_out(log1) == fp32_out(log0) + 1, (log1.counts, log0.counts)
    compare((on, off), clouds, tap, active=True)


def test_full_size_fp32_maps(full, tap):
    """the same batch with fp32 dense maps (pair_rows_dense off): window_conv_f16_kernel on fp32 rows, the row-wave kernel on fp32 rows"""
    cfg, sd, _, _, batch, clouds = full
    engines = pair(dataclasses.replace(cfg, pair_rows_dense=False), sd)
    compare(engines, clouds, tap, active=True)


def test_return_intermediates_keeps_the_full_head_rows(full):
    cfg, sd, on, off, batch, clouds = full
    r1, it1 = on.forward(clouds, return_intermediates=True)
    assert not on.last_head_at_peaks
    r0, it0 = off.forward(clouds, return_intermediates=True)
    n_head = max(c0 + n for c0, n in on.head_slices.values())          # (the rows' padding columns are never written)
    assert it1["head_rows"].shape == it0["head_rows"].shape and it1["head_rows"].shape[1] == on.head_ld
    assert torch.equal(it1["head_rows"][:, :n_head], it0["head_rows"][:, :n_head])
    assert_same_results(r1, r0)
    # ... and the stages called on their own
    _, h, w = on._final_shape()
    _, rows = on.bev_and_head(it0["spatial_features_nhwc"], batch, h, w)
    assert torch.is_tensor(rows) and rows.shape == it0["head_rows"].shape


def test_range_guard_rerun_matches(full, tap):
    """a step whose activations leave fp16's range is re-run guarded (fp32 rows, pre-scaled inputs): the peaks path runs in the re-run too"""
    cfg, sd, _, _, batch, clouds = full
    hot = dict(sd)
    hot["backbone_3d.conv_input.1.weight"] = sd["backbone_3d.conv_input.1.weight"] * 3e4
    hot["backbone_3d.conv_input.1.bias"] = sd["backbone_3d.conv_input.1.bias"] * 3e4
    # (the sparse backbone runs 3e4 times hotter, past 2^15; its last BatchNorm brings the dense half back to ordinary magnitudes, so
    # that the head's outputs -- exp() of the size channels -- stay where an absolute box tolerance means something)
    hot["backbone_3d.conv_out.1.weight"] = sd["backbone_3d.conv_out.1.weight"] / 3e4
    on, off = pair(cfg, hot)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r1 = on.forward(clouds)
        d1 = tap.pop()
        r0 = off.forward(clouds)
        d0 = tap.pop()
    assert on.range_reruns == off.range_reruns == 1 and on.last_head_at_peaks
    assert sum(len(r["pred_boxes"]) for r in r0) > 10 and all(float(r["pred_boxes"].abs().max()) < 1e3 for r in r0 if len(r["pred_boxes"]))
    assert_same_results(r1, r0)
    assert_same_decode(d1, d0, cfg.nms_thresh)


def test_two_stage_engine_gets_the_peaks_path(full):
    from cpd_amd.two_stage import VoxelRCNNEngine
    cfg, sd, _, _, batch, clouds = full
    mcfg = models.waymo_voxel_rcnn_cfg()
    torch.manual_seed(0)
    head = models.__all__[mcfg.ROI_HEAD.NAME](input_channels={"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 128}, model_cfg=mcfg.ROI_HEAD,
                                              point_cloud_range=cfg.point_cloud_range, voxel_size=cfg.voxel_size, num_class=1)
    with torch.no_grad():
        head.cls_layers[-1].weight.normal_(0, 0.3); head.cls_layers[-1].bias.normal_(0, 0.3)
        head.reg_layers[-1].weight.normal_(0, 0.01); head.reg_layers[-1].bias.zero_()
    sd2 = dict(sd)
    sd2.update({"roi_head." + k: v.detach().clone() for k, v in head.state_dict().items()})
    on, off = (VoxelRCNNEngine(dataclasses.replace(cfg, head_at_peaks=flag, head_at_peaks_min_frames=1), mcfg.ROI_HEAD, mcfg.POST_PROCESSING, sd2) for flag in (True, False))
    (r1, it1), (r0, it0) = on.forward(clouds, return_intermediates=True), off.forward(clouds, return_intermediates=True)
    assert on.rpn.last_head_at_peaks and not off.rpn.last_head_at_peaks
    # ---- the proposals are the decode's product: the rule applies to them as it stands
    assert it1["rois"].shape == it0["rois"].shape and it0["rois"].shape[1] > 100
    assert torch.equal(it1["roi_scores"], it0["roi_scores"]) and torch.equal(it1["roi_labels"], it0["roi_labels"])
    assert float(_box_err(it1["rois"], it0["rois"]).max()) <= BOX_ATOL
    # ---- the second stage is the same function in both engines: same pooled levels bit for bit, and the full-map engine's second stage
    # run on the peaks engine's proposals returns the peaks engine's detections bit for bit
    for name in it0["levels"]:
        assert torch.equal(it1["levels"][name][0], it0["levels"][name][0]) and torch.equal(it1["levels"][name][1], it0["levels"][name][1])
    own = on.forward(clouds)
    rpn0, off.rpn = off.rpn, on.rpn
    try:
        crossed = off.forward(clouds)
    finally:
        off.rpn = rpn0
    for g, w in zip(crossed, own):
        assert all(torch.equal(g[k], w[k]) for k in ("pred_boxes", "pred_scores", "pred_labels"))
    # ---- so every difference downstream comes from proposals that moved by <= 1e-4 (above). RoI by RoI, before the final NMS (the RoIs
    # of the two runs are aligned: identical proposal scores). The pooling is continuous in the proposal EXCEPT where a voxel enters or
    # leaves a grid point's neighbour set (the query's radius test): there one grid point's pooled features jump by the size of a
    # feature, elsewhere they move by the proposal's move times the position MLP's gain. The test SHOWS the cause for every RoI it
    # exempts: its pooled features differ by more than 1e-3 in some grid point (measured: the continuous moves are <= 2.2e-4, the jumps
    # >= 1e-2, nothing in between; 10 of 1500 RoIs jump). Every other RoI must agree to the contract: class logits within 1e-4 of the
    # outputs' scale, boxes within the proposals' 1e-4 plus the stage's own 1e-4.
    n_roi = it0["rois"].shape[1]
    jump = (it1["pooled"] - it0["pooled"]).abs().amax(dim=(1, 2)).view(batch, n_roi)
    moved = jump > 1e-3
    scale = max(1.0, float(it0["batch_cls_preds"].abs().max()))
    d_cls = (it1["batch_cls_preds"] - it0["batch_cls_preds"]).abs().view(batch, n_roi)
    d_box = _box_err(it1["batch_box_preds"], it0["batch_box_preds"]).amax(-1)
    print("two-stage: %d of %d RoIs with a changed neighbour set; elsewhere max |logit diff| %.3g (scale %.3g), max |box diff| %.3g; "
          "at the changed ones %.3g / %.3g" % (int(moved.sum()), moved.numel(), float(d_cls[~moved].max()), scale, float(d_box[~moved].max()),
                                               float(d_cls[moved].max()) if moved.any() else 0.0, float(d_box[moved].max()) if moved.any() else 0.0))
    assert int(moved.sum()) <= 0.02 * moved.numel()            # (a radius test decided within 1e-4 of its threshold: rare by geometry)
    assert float(d_cls[~moved].max()) <= 1e-4 * scale and float(d_box[~moved].max()) <= 2 * BOX_ATOL
    # ---- the final detections (sorted by scores that saturate at 1.0f: ties change places, so they are matched by geometry): every
    # detection has its counterpart -- same label, box within 2e-4, score within sigmoid's slope (1/4) times the logit bound -- except
    # as many per frame as that frame has RoIs with a changed neighbour set (each can change itself and, through the NMS, one other)
    assert len(r1) == len(r0) and sum(len(r["pred_boxes"]) for r in r0) > 10
    for f, (g, w) in enumerate(zip(r1, r0)):
        allow = 2 * int(moved[f].sum())
        assert abs(len(g["pred_boxes"]) - len(w["pred_boxes"])) <= allow
        d = _box_err(g["pred_boxes"][:, None, :], w["pred_boxes"][None, :, :]).amax(-1)
        same = (d <= 2 * BOX_ATOL) & ((g["pred_scores"][:, None] - w["pred_scores"][None, :]).abs() <= 0.25e-4 * scale) & \
               (g["pred_labels"][:, None] == w["pred_labels"][None, :])
        lone = int((~same.any(1)).sum())
        print("two-stage frame %d: %d detections, %d without a counterpart (allowed %d)" % (f, len(d), lone, allow))
        assert lone <= allow and int((~same.any(0)).sum()) <= allow


def test_anchor_engine_is_unaffected(hip):
    from cpd_amd.anchor_engine import AnchorPointEngine, synthetic_two_stage_state
    cfg = small_cfg()
    mcfg, sd = synthetic_two_stage_state(cfg, init_state_dict(cfg, 0), seed=1)
    clouds = small_clouds(2)
    outs = []
    for flag in (True, False):
        rpn = AnchorPointEngine(dataclasses.replace(cfg, head_at_peaks=flag, head_at_peaks_min_frames=1), sd, mcfg.DENSE_HEAD,
                                mcfg.ROI_HEAD.NMS_CONFIG["TEST"])
        outs.append(rpn.forward(clouds, proposals=["x_conv3", "x_conv4"]))
        assert not rpn.last_head_at_peaks
    (b1, s1, l1, n1, _), (b0, s0, l0, n0, _) = outs
    assert n1 == n0 and sum(n0) > 10
    for f, n in enumerate(n0):
        assert torch.equal(b1[f, :n], b0[f, :n]) and torch.equal(s1[f, :n], s0[f, :n]) and torch.equal(l1[f, :n], l0[f, :n])


def test_environment_switch(hip, monkeypatch):
    cfg = small_cfg()
    sd = init_state_dict(cfg, seed=1)
    monkeypatch.setenv("CPD_HEAD_AT_PEAKS", "0")
    assert not CenterPointEngine(cfg, sd).head_at_peaks
    monkeypatch.setenv("CPD_HEAD_AT_PEAKS", "1")
    assert CenterPointEngine(cfg, sd).head_at_peaks
    assert not CenterPointEngine(dataclasses.replace(cfg, head_at_peaks=False), sd).head_at_peaks
