"""GPU: cpd_recall_record (csrc/iou3d_nms.hip) and everything built on it -- cpd_amd.recall.RecallRecord / generate_recall_record,
CenterPoint / VoxelRCNN.post_processing, VoxelRCNNEngine.forward(recall=) -- against the reference's own method (tests/golden/recall.npz),
the numpy restatement (tests/ref_recall.py) and the IoU matrix of cpd_boxes_iou3d on the same device."""
import numpy as np
import pytest

import ref_recall as R

pytestmark = pytest.mark.gpu
THRESH = [0.3, 0.5, 0.7]
CASES = ("plain", "one", "twice", "zero", "empty")
REF_ORDER = ["gt", "roi_0.3", "rcnn_0.3", "roi_0.5", "rcnn_0.5", "roi_0.7", "rcnn_0.7"]       # as the reference inserts its keys
ROWS_PER_WAVE, ROWS_PER_BLOCK = 4, 64           # RECALL_ROWS, RECALL_WAVES * RECALL_ROWS of csrc/iou3d_nms.hip


@pytest.fixture(scope="module")
def rz(golden):
    return golden("recall")


def case_inputs(rz, name):
    preds = R.split(rz[name + "_pred"], rz[name + "_pred_n"])
    rois = rz[name + "_rois"] if name + "_rois" in rz.files else None
    return preds, rois, rz[name + "_gt"]


def case_start(rz, name):
    return rz["plain_dicts"][-1].copy() if name == "twice" else np.zeros(7, np.int64)


def cuda(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def addressed(frames, form, ld=7, filler=None):
    """per-frame [n_b, 7] arrays -> (rows, start, count) device tensors: form 'block' = a padded [B, cap, ld] block whose slots past
    a frame's count hold `filler` (a box that would change the result if it were read), 'concat' = the frames one after another behind
    two leading rows of filler"""
    b = len(frames)
    ns = [len(f) for f in frames]
    fill = np.zeros(ld, np.float32) if filler is None else np.concatenate([filler[:7], np.zeros(ld - 7, np.float32)])
    if form == "block":
        cap = max(ns) + 1
        rows = np.tile(fill, (b, cap, 1)).astype(np.float32)
        for i, f in enumerate(frames):
            rows[i, :ns[i], :7] = f[:, :7]
            rows[i, :ns[i], 7:] = 5.0                      # extra columns are never read
        start = np.arange(b) * cap
    else:
        rows = np.tile(fill, (2 + sum(ns), 1)).astype(np.float32)
        start = 2 + np.concatenate([[0], np.cumsum(ns)[:-1]])
        for i, f in enumerate(frames):
            rows[start[i]:start[i] + ns[i], :7] = f[:, :7]
            rows[start[i]:start[i] + ns[i], 7:] = 5.0
    return cuda(rows), cuda(start, np.int32), cuda(ns, np.int32)


def run_abi(preds, gts, rois, thresh, form="concat", ld=7, counters=None):
    """cpd_recall_record through cpd_amd.ops -> (counters, best_rcnn, best_roi, n_gt) as numpy"""
    import torch
    from cpd_amd import ops
    gt = cuda(gts)
    b, m = gt.shape[:2]
    filler = gts[0, 0] if m else None
    p, ps, pc = addressed(preds, form, ld, filler)
    r = rs = rc = None
    if rois is not None:
        r, rs, rc = addressed(list(rois), form, ld, filler)
    if counters is None:
        counters = torch.zeros(1 + 2 * len(thresh), dtype=torch.int64, device="cuda")
    br = torch.full((b, m), 7.0, device="cuda")
    bo = torch.full((b, m), 7.0, device="cuda")
    ng = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    ops.recall_record(p, ps, pc, gt, thresh, counters, rois=r, roi_start=rs, roi_count=rc, best_rcnn=br, best_roi=bo, n_gt=ng)
    return counters.cpu().numpy(), br.cpu().numpy(), bo.cpu().numpy(), ng.cpu().numpy()


# ---- the golden cases (the reference's own method) through every entry --------------------------------------------------

@pytest.mark.parametrize("form", ["concat", "block"])
@pytest.mark.parametrize("name", CASES)
def test_abi_on_the_golden_cases(hip, rz, name, form):
    preds, rois, gts = case_inputs(rz, name)
    c, br, bo, ng = run_abi(preds, gts, rois, THRESH, form)
    assert np.array_equal(c + case_start(rz, name), rz[name + "_dicts"][-1])
    assert np.array_equal(ng, rz[name + "_ngt"])
    if gts.shape[1]:
        assert np.abs(br - rz[name + "_best_rcnn"]).max() <= 1e-4
        assert np.abs(bo - rz[name + "_best_roi"]).max() <= 1e-4


@pytest.mark.parametrize("name", CASES)
def test_generate_recall_record_on_the_golden_cases(hip, rz, name):
    """the reference's static method, frame by frame on one dict: the dict after EVERY frame is the reference's"""
    import torch
    from cpd_amd import models, recall
    preds, rois, gts = case_inputs(rz, name)
    keys = [str(k) for k in rz["keys"]]
    data = {"gt_boxes": cuda(gts)}
    if rois is not None:
        data["rois"] = cuda(rois)
    d = {}
    if name == "twice":                                           # goes on from the dict the plain case left
        start = dict(zip(keys, (int(v) for v in case_start(rz, name))))
        d = {k: start[k] for k in REF_ORDER}
    fn = (recall.generate_recall_record, models.CenterPoint.generate_recall_record, models.VoxelRCNN.generate_recall_record)
    for f in range(len(gts)):
        d = fn[f % 3](box_preds=cuda(preds[f]).reshape(-1, 7), recall_dict=d, batch_index=f, data_dict=data, thresh_list=THRESH)
        assert list(d) == REF_ORDER and all(type(v) is int for v in d.values())
        assert [d[k] for k in keys] == list(rz[name + "_dicts"][f])
    assert recall.generate_recall_record(torch.zeros(0, 7).cuda(), {}, 0, {"rois": 1}, THRESH) == {}      # no gt_boxes: the dict as given


@pytest.mark.parametrize("name", CASES)
def test_recall_record_on_the_golden_cases(hip, rz, name):
    """RecallRecord.update in its three input forms: a list of per-frame tensors, a concatenation, a padded block with device counts"""
    from cpd_amd.recall import RecallRecord
    preds, rois, gts = case_inputs(rz, name)
    keys = [str(k) for k in rz["keys"]]
    want = dict(zip(keys, (int(v) for v in rz[name + "_dicts"][-1])))
    roi_dev = None if rois is None else cuda(rois)
    for form in ("list", "concat", "block"):
        rec = RecallRecord(THRESH).load_counts(case_start(rz, name))
        if form == "list":
            out = rec.update([cuda(p).reshape(-1, 7) for p in preds], None, None, cuda(gts), rois=roi_dev)
        else:
            p, ps, pc = addressed(preds, form, 9, gts[0, 0] if gts.shape[1] else None)
            out = rec.update(p, ps if form == "concat" else None, pc, cuda(gts), rois=roi_dev)
        assert out is None
        assert rec.as_dict() == want and list(rec.as_dict()) == REF_ORDER
        gt = max(want["gt"], 1)
        assert rec.summary() == {k2: v for t in THRESH for k2, v in (("recall/roi_%s" % t, want["roi_%s" % t] / gt),
                                                                    ("recall/rcnn_%s" % t, want["rcnn_%s" % t] / gt))}


@pytest.fixture(scope="module")
def two_stage_net(hip):
    import torch
    from cpd_amd import models
    cfg = models.waymo_voxel_rcnn_cfg()
    cfg.BACKBONE_2D.NUM_FILTERS, cfg.BACKBONE_2D.NUM_UPSAMPLE_FILTERS, cfg.BACKBONE_2D.LAYER_NUMS = [64, 128], [128, 128], [2, 2]
    cfg.DENSE_HEAD.POST_PROCESSING.POST_CENTER_LIMIT_RANGE = [-20, -20, -2, 20, 20, 4]
    cfg.DENSE_HEAD.POST_PROCESSING.MAX_OBJ_PER_SAMPLE = 100
    torch.manual_seed(3)
    net = models.VoxelRCNN(cfg, point_cloud_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 4.0]).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.75, 1.25)
                m.weight.uniform_(0.75, 1.25); m.bias.normal_(0, 0.1)
        for stack in (net.roi_head.cls_layers, net.roi_head.reg_layers):       # spread the scores, so that the final NMS has work
            stack[-1].weight.normal_(0, 0.3); stack[-1].bias.normal_(0, 0.3)
    return net


@pytest.mark.parametrize("name", ["plain", "one", "zero", "empty"])
def test_post_processing_on_hand_filled_batch_dicts(hip, rz, two_stage_net, name):
    """VoxelRCNN.post_processing (final boxes = the golden frames' boxes: logits far above the score threshold, padding far below,
    an NMS threshold no IoU exceeds) and CenterPoint.post_processing (final_box_dicts given); both return {} without gt_boxes."""
    import torch
    from cpd_amd import models
    preds, rois, gts = case_inputs(rz, name)
    keys = [str(k) for k in rz["keys"]]
    want = dict(zip(keys, (int(v) for v in rz[name + "_dicts"][-1])))
    b, n = len(preds), max(1, max(len(p) for p in preds))
    boxes, cls = np.zeros((b, n, 7), np.float32), np.full((b, n, 1), -20.0, np.float32)
    boxes[:, :, 3:6] = 1.0
    for f, p in enumerate(preds):
        boxes[f, :len(p)], cls[f, :len(p)] = p, 6.0
    net = two_stage_net
    nms = net.model_cfg.POST_PROCESSING.NMS_CONFIG
    old = nms["NMS_THRESH"]
    nms["NMS_THRESH"] = 2.0
    try:
        bd = dict(batch_size=b, batch_box_preds=cuda(boxes), batch_cls_preds=cuda(cls), cls_preds_normalized=False, has_class_labels=True,
                  roi_labels=torch.ones(b, n, dtype=torch.int64, device="cuda"))
        assert net.post_processing(dict(bd))[1] == {}
        bd["gt_boxes"] = cuda(gts)
        if rois is not None:
            bd["rois"] = cuda(rois)
        pred_dicts, rec = net.post_processing(bd)
    finally:
        nms["NMS_THRESH"] = old
    assert [len(d["pred_boxes"]) for d in pred_dicts] == [len(p) for p in preds]
    if rois is None:                                              # (a two-stage batch always has rois; without them the roi keys stay 0)
        assert all(rec[k] == 0 for k in rec if k.startswith("roi_"))
    assert rec == want and list(rec) == REF_ORDER
    one = models.CenterPoint.post_processing(net, {"final_box_dicts": [{"pred_boxes": cuda(p).reshape(-1, 7)} for p in preds], "batch_size": b})
    assert one[1] == {}
    fd = {"final_box_dicts": [{"pred_boxes": cuda(p).reshape(-1, 7)} for p in preds], "batch_size": b, "gt_boxes": cuda(gts)}
    got_preds, rec1 = models.CenterPoint.post_processing(net, fd)
    assert got_preds is fd["final_box_dicts"]
    assert rec1 == dict(zip(keys, (int(v) for v in rz[("one" if name == "plain" else name) + "_dicts"][-1])))


# ---- tile edges: against the restatement and against cpd_boxes_iou3d on the same device -----------------------------------

def grid_boxes(rng, n, cells=12, pitch=9.0):
    pick = rng.permutation(cells * cells)[:n]
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = (pick % cells - cells / 2) * pitch + rng.uniform(-1, 1, n)
    b[:, 1] = (pick // cells - cells / 2) * pitch + rng.uniform(-1, 1, n)
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3:6] = np.exp(rng.normal(0, 0.2, (n, 3))) * np.array([4.7, 2.1, 1.7])
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def near(rng, gt, n):
    """n boxes: jittered copies of randomly drawn gts (IoUs from about 0.9 down to 0) and a few unrelated ones"""
    if n == 0:
        return np.zeros((0, 7), np.float32)
    src = gt[rng.integers(0, len(gt), n), :7].astype(np.float64)
    s = rng.choice([0.03, 0.1, 0.2, 0.4, 0.8], n)[:, None]
    src[:, :2] += rng.normal(0, 1.5, (n, 2)) * s
    src[:, 2] += rng.normal(0, 0.3, n) * s[:, 0]
    src[:, 3:6] *= np.exp(rng.normal(0, 0.25, (n, 3)) * s)
    src[:, 6] += rng.normal(0, 0.4, n) * s[:, 0]
    return src.astype(np.float32)


E = (ROWS_PER_WAVE, ROWS_PER_BLOCK)
# (real gts per frame, final boxes per frame, RoIs per frame or None, gt_ld, thresholds, form)
TILE_CASES = [
    ([1], [0], [1], 7, [0.5], "block"),
    ([63], [E[0] - 1], [E[1] + 1], 8, THRESH, "concat"),
    ([64], [E[0]], None, 7, THRESH, "block"),
    ([65], [E[0] + 1], [E[1]], 8, [0.0, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9], "concat"),
    ([129], [E[1] - 1], [1], 7, THRESH, "block"),
    ([1, 65, 64], [E[1] + 1, 0, E[0]], [E[0] + 1, E[1] - 1, 0], 8, THRESH, "block"),
    ([129, 63, 5], [1, E[1], E[0] - 1], [E[1] + E[0], 2, E[0]], 7, [0.0, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9], "concat"),
    ([64, 1, 65], [E[0] + 1, E[1] + 1, 1], None, 8, [0.7], "concat"),
    ([5, 129, 63], [0, E[1] - 1, 2 * E[1] + 1], [0, 0, 3], 7, THRESH, "block"),
]


@pytest.mark.parametrize("case", range(len(TILE_CASES)))
def test_tile_edges_match_the_restatement_and_the_iou_kernel(hip, oracle, case):
    import torch
    from cpd_amd import ops
    n_gt, n_pred, n_roi, ld, thresh, form = TILE_CASES[case]
    rng = np.random.default_rng(100 + case)
    b, cap = len(n_gt), max(n_gt)
    gts = np.zeros((b, cap, ld), np.float32)
    preds, rois = [], (None if n_roi is None else [])
    for f in range(b):
        g = grid_boxes(rng, n_gt[f])
        gts[f, :n_gt[f], :7] = g
        if ld == 8:
            gts[f, :n_gt[f], 7] = rng.integers(1, 4, n_gt[f])
        preds.append(near(rng, g, n_pred[f]))
        if rois is not None:
            rois.append(near(rng, g, n_roi[f]))
    c, br, bo, ng = run_abi(preds, gts, rois, thresh, form, ld=7 + case % 3)
    rc, rbr, rbo, rng_ = R.batch_record(oracle, preds, gts, rois, thresh)
    print("case %d: counters %s, restatement %s" % (case, c.tolist(), rc.tolist()))
    assert np.array_equal(ng, rng_) and list(ng) == n_gt and c[0] == sum(n_gt)
    print("max |best - restatement| = %.3g / %.3g" % (np.abs(br - rbr).max(), np.abs(bo - rbo).max()))
    assert np.abs(br - rbr).max() <= 1e-4 and np.abs(bo - rbo).max() <= 1e-4
    # ... and EQUAL to what the pinned cpd_boxes_iou3d kernel gives on this device: its column maxima, its thresholded counts
    want = np.zeros_like(c)
    want[0] = sum(n_gt)
    t = len(thresh)
    for side, (boxes, best) in enumerate(((rois, bo), (preds, br))):
        for f in range(b):
            col = np.full(cap, -1.0, np.float32)
            if boxes is not None and len(boxes[f]):
                iou = ops.boxes_iou3d(cuda(boxes[f]), cuda(gts[f, :n_gt[f], :7])).cpu().numpy()
                col[:n_gt[f]] = iou.max(axis=0)
                for k, thr in enumerate(thresh):
                    want[1 + side * t + k] += int((col[:n_gt[f]] > np.float32(thr)).sum())
            assert np.array_equal(best[f], col), "frame %d side %d: max |diff| %.3g" % (f, side, np.abs(best[f] - col).max())
    assert np.array_equal(c, want)
    assert c[1:].sum() > 0                                        # the case is not vacuous: something is recalled
    torch.cuda.synchronize()


def test_two_updates_equal_the_sum_of_the_single_updates(hip, rz):
    import torch
    p1, r1, g1 = case_inputs(rz, "plain")
    p2, r2, g2 = case_inputs(rz, "twice")
    a = run_abi(p1, g1, r1, THRESH)[0]
    b = run_abi(p2, g2, r2, THRESH)[0]
    acc = torch.zeros(7, dtype=torch.int64, device="cuda")
    run_abi(p1, g1, r1, THRESH, counters=acc)
    both = run_abi(p2, g2, r2, THRESH, "block", counters=acc)[0]
    assert np.array_equal(both, a + b) and np.array_equal(both, rz["twice_dicts"][-1])
    assert a[0] > 0 and b[0] > 0


def test_bad_arguments_give_err_arg(hip):
    import ctypes
    import torch
    from cpd_amd import _lib
    lib, P = _lib.lib(), _lib.ptr
    pred, gt6, gt8 = torch.zeros(4, 7).cuda(), torch.zeros(1, 3, 6).cuda(), torch.zeros(1, 3, 8).cuda()
    st, ct = torch.zeros(1, dtype=torch.int32).cuda(), torch.full((1,), 4, dtype=torch.int32).cuda()
    counters = torch.zeros(17, dtype=torch.int64).cuda()

    def call(gt, ld, thresh, n_thresh):
        th = (ctypes.c_float * 9)(*thresh)
        return lib.cpd_recall_record(P(pred), 7, P(st), P(ct), None, 0, None, None, P(gt), 1, 3, ld, th, n_thresh, P(counters), None, None,
                                     None, _lib.stream())
    ok = [0.3, 0.5, 0.7, 0.1, 0.2, 0.4, 0.6, 0.8, 0.9]
    assert call(gt8, 8, ok, 0) == -1 and call(gt8, 8, ok, 9) == -1
    assert call(gt8, 8, [0.3, -0.5] + ok[2:], 3) == -1
    assert call(gt6, 6, ok, 3) == -1
    assert call(gt8, 8, ok, 3) == 0 and call(gt8, 8, ok, 8) == 0 and call(gt8, 8, ok, 1) == 0
    torch.cuda.synchronize()
    assert counters.tolist() == [3] + [0] * 16                    # three good calls, one all-zero gt block each: nothing else touched


# ---- the fused two-stage engine ---------------------------------------------------------------------------------------------

def test_engine_with_a_record_returns_the_same_detections_and_the_frame_by_frame_record(hip, two_stage_net):
    import torch
    from cpd_amd import recall
    from cpd_amd.synthetic import waymo_cloud
    clouds = []
    for s_ in (0, 1, 2):
        p = waymo_cloud(s_, n_points=40000 + 5000 * s_)
        p[:, :2] *= 0.3
        clouds.append(torch.from_numpy(p).cuda())
    eng = two_stage_net.to_engine()
    plain, it = eng.forward(clouds, return_intermediates=True)
    assert sum(len(d["pred_boxes"]) for d in plain) > 10 and it["rois"].shape[1] > 10
    # gts: every third RoI of a frame, shifted by about a tenth of its size
    g = torch.Generator().manual_seed(1)
    per_frame = []
    for b in range(3):
        r = it["rois"][b].cpu()
        r = r[r[:, 3] > 0][::3, :7].clone()
        r[:, :2] += torch.randn(len(r), 2, generator=g) * 0.1 * r[:, 3:5]
        per_frame.append(torch.cat([r, torch.ones(len(r), 1)], dim=1)[:len(r) - b])
    gt = recall.pad_gt(per_frame).cuda()
    rec = recall.RecallRecord(THRESH)
    got, it2 = eng.forward(clouds, return_intermediates=True, gt_boxes=gt, recall=rec)
    for a, w in zip(got, plain):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(a[k], w[k])
    assert torch.equal(it2["rois"], it["rois"])
    want = {}
    data = {"gt_boxes": gt, "rois": it2["rois"]}
    for b in range(3):
        want = recall.generate_recall_record(got[b]["pred_boxes"], want, b, data, THRESH)
    d = rec.as_dict()
    assert d == want and d["gt"] == sum(len(x) for x in per_frame) > 0
    assert 0 < d["roi_0.3"] <= d["gt"] and d["roi_0.7"] <= d["roi_0.5"] <= d["roi_0.3"]
    eng.forward(clouds, return_intermediates=True, gt_boxes=gt, recall=rec)            # a second step accumulates
    assert rec.as_dict() == {k: 2 * v for k, v in want.items()}
    # the default step (pooled levels kept as fp16-pair rows): the same detections with and without a record
    base = eng.forward(clouds)
    with_rec = eng.forward(clouds, gt_boxes=gt, recall=recall.RecallRecord(THRESH))
    for a, w in zip(with_rec, base):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(a[k], w[k])
