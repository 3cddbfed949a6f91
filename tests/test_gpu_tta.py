"""Test-time augmentation in one device step (csrc/tta.hip, cpd_amd/tta.py) on the GPU: cpd_tta_views against TestAugmentor.forward,
cpd_tta_collect against its host build, collect + fusion against wbf._merge, and TTAEngine against the host composition it replaces
(TestAugmentor.forward per view, one engine step, TestAugmentor.backward on the host, wbf.merge_frames)."""
import numpy as np
import pytest
import torch

import ref_tta as RT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def T(hip):
    from cpd_amd import tta
    return tta


def dev(case):
    return [torch.from_numpy(case[k].copy()).to(DEV) for k in ("boxes", "scores", "labels", "counts")]


# 1. the views
@pytest.mark.parametrize("sizes,c", [((0, 1, 2051), 5), ((777,), 4)])
def test_views_are_test_augmentor_forward(T, sizes, c):
    rng = np.random.default_rng(sum(sizes) + c)
    frames = [torch.from_numpy((rng.normal(size=(n, c)) * np.array([40, 40, 2] + [1] * (c - 3))).astype(np.float32)).to(DEV) for n in sizes]
    augs = RT.augmentors(RT.EIGHT)
    got = T.views(frames, augs)
    assert len(got) == len(augs) * len(frames)
    for v, aug in enumerate(augs):
        for f, pts in enumerate(frames):
            want = aug.forward(dict(points=pts.clone()))["points"]
            g = got[v * len(frames) + f]
            assert g.shape == want.shape == pts.shape
            assert g.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (v, f)
    if len(sizes) > 1:                       # the list is slices of ONE view-major block
        n_total = sum(sizes)
        assert all(g.untyped_storage().data_ptr() == got[0].untyped_storage().data_ptr() for g in got)
        assert got[len(frames) + 2].storage_offset() == (n_total + sizes[0] + sizes[1]) * c


# 2. collect: the device entry point against its host build
@pytest.mark.parametrize("name", ["segment", "backward"])
def test_collect_is_bit_equal_to_its_host_build(T, name):
    case = RT.segment_case() if name == "segment" else RT.backward_case()
    merge, classes = (RT.MERGE, RT.CLASSES) if name == "segment" else (dict(WBF_IOUS=[0.5], WBF_PRE_SCORES=[-1.0], MERGE_TYPE=["NMS"], NMS_IOU=0.1), RT.CLASSES[:1])
    augs = RT.augmentors(RT.EIGHT)
    want = T.collect_cpu(*[torch.from_numpy(case[k].copy()) for k in ("boxes", "scores", "labels", "counts")], augs, merge, classes, case["batch"])
    got = T.collect(*dev(case), augs, merge, classes, case["batch"])
    for field, g, w in zip(T.Segments._fields, got, want):
        assert g.cpu().numpy().tobytes() == w.numpy().tobytes(), field
    if name == "segment":
        assert int(got.count.min()) == -1 and int(got.count.max()) == RT.MAX_SEGMENT
        with pytest.raises(ValueError, match="refused a segment"):
            T.fuse(got, merge, classes, case["batch"])


# 3. collect + fusion against wbf._merge on the device-written boxes
def forward_boxes(world, rot, axis):
    """what a detector would see of `world` through a shipped view (float64; the views come back nudged anyway)"""
    b = world.astype(np.float64).copy()
    c, s = np.cos(rot), np.sin(rot)
    b[:, 0], b[:, 1] = world[:, 0] * c - world[:, 1] * s, world[:, 0] * s + world[:, 1] * c
    b[:, 6] += rot
    if axis == "x":
        b[:, 1], b[:, 6] = -b[:, 1], -b[:, 6]
    return b


@pytest.fixture(scope="module")
def fusion_case():
    """six shipped views of B = 2 frames; frame 0: 600 separate objects of class 0 (more clusters than CPD_WBF_LDS_CLUSTERS), 150 of
    class 1 (NMS) and 150 of class 2; frame 1: 40 / 30 / 30. Every view sees every object, nudged, with its own score."""
    import ref_augment as RA
    rng = np.random.default_rng(20263)
    n_views, batch, cap = 6, 2, 900
    boxes = np.zeros((n_views * batch, cap, 7), np.float32)
    scores = np.zeros((n_views * batch, cap), np.float32)
    labels = np.zeros((n_views * batch, cap), np.int64)
    counts = np.zeros((n_views * batch,), np.int32)
    for f, per_class in enumerate(((600, 150, 150), (40, 30, 30))):
        n = sum(per_class)
        side = int(np.ceil(np.sqrt(n)))
        gx, gy = np.meshgrid(np.arange(side), np.arange(side))
        world = np.zeros((n, 7))
        world[:, 0], world[:, 1] = (gx.reshape(-1)[:n] - side / 2) * 4.0, (gy.reshape(-1)[:n] - side / 2) * 4.0
        world[:, 3:6] = rng.uniform([1.5, 0.8, 1.0], [3.0, 1.6, 2.0], (n, 3))
        world[:, 6] = rng.uniform(-3, 3, n)
        lab = np.repeat([1, 2, 3], per_class)
        distinct = (0.05 + 0.95 * (rng.permutation(n_views * n) + 0.5) / (n_views * n)).astype(np.float32).reshape(n_views, n)
        for v, (rot, axis) in enumerate(RA.TEST_VIEWS):
            seen = forward_boxes(world, rot, axis) + rng.normal(size=(n, 7)) * [0.08, 0.08, 0.03, 0.05, 0.03, 0.03, 0.03]
            order = rng.permutation(n)
            i = v * batch + f
            boxes[i, :n], labels[i, :n], counts[i] = seen[order], lab[order], n
            scores[i, :n] = distinct[v]
    for f in range(batch):                    # no ties within a frame: nms_gpu's own argsort leaves them open
        assert len(np.unique(scores[f::batch][scores[f::batch] > 0])) == counts[f::batch].sum()
    return dict(n_views=n_views, batch=batch, cap=cap, boxes=boxes, scores=scores, labels=labels, counts=counts)


def test_fusion_is_wbf_merge_on_the_device_written_boxes(T, fusion_case):
    from cpd_amd import wbf
    case = fusion_case
    n_views, batch, cap, n_class = case["n_views"], case["batch"], case["cap"], len(RT.CLASSES)
    augs = RT.augmentors(RT.SHIPPED)
    seg = T.collect(*dev(case), augs, RT.MERGE, RT.CLASSES, batch)
    got = T.fuse(seg, RT.MERGE, RT.CLASSES, batch)
    # the device-written backward boxes, read back and put at their slots
    back = np.full((batch, n_views * cap, 7), np.nan, np.float32)
    src, cnt, sb = seg.src.cpu().numpy(), seg.count.cpu().numpy(), seg.boxes.cpu().numpy()
    for s in range(batch * n_class):
        back[s // n_class, src[s, :cnt[s]]] = sb[s, :cnt[s]]
    back = back.reshape(batch, n_views, cap, 7).transpose(1, 0, 2, 3).reshape(n_views * batch, cap, 7)
    frames = [(n, s, b) for n, s, b, _ in RT.frame_lists(RT.label_names(case["labels"]), case["scores"], back, case["counts"], n_views, batch)]
    want = wbf._merge(frames, RT.MERGE, RT.CLASSES, None, None)
    names = np.array(RT.CLASSES)
    for f in range(batch):
        wn, ws, wb = want[f]
        assert names[got[f]["pred_labels"].cpu().numpy() - 1].tolist() == wn.tolist()
        assert got[f]["pred_scores"].cpu().numpy().tobytes() == ws.tobytes()
        assert got[f]["pred_boxes"].cpu().numpy().tobytes() == np.ascontiguousarray(wb).tobytes()
        assert not np.isnan(wb).any()
    n0 = int((want[0][0] == RT.CLASSES[0]).sum())
    assert wbf.LDS_CLUSTERS < n0 < cnt[0], n0                                    # clusters beyond LDS, and views did fuse
    assert set(want[0][0].tolist()) == set(RT.CLASSES) and (cnt > 0).all()


# 4. end to end
def composition(engine, augs, clouds, merge, classes):
    """the host composition on the same view-major batch: TestAugmentor.forward per view, ONE engine step, TestAugmentor.backward on the
    host, wbf.merge_frames -> (per (view, frame) box counts, merged infos)"""
    from cpd_amd import wbf
    b = len(clouds)
    res = engine.forward([a.forward(dict(points=p.clone()))["points"] for a in augs for p in clouds])
    names = np.array(classes)
    infos = [[dict(name=names[res[v * b + f]["pred_labels"].cpu().numpy() - 1], score=res[v * b + f]["pred_scores"].cpu().numpy(),
                   boxes_lidar=a.backward(dict(boxes_lidar=res[v * b + f]["pred_boxes"].cpu().numpy().copy()))["boxes_lidar"])
              for f in range(b)] for v, a in enumerate(augs)]
    return [len(r["pred_scores"]) for r in res], wbf.merge_frames(infos, merge, classes, _nms=nms_in_segment_order)


def nms_in_segment_order(boxes, scores, thresh):
    """wbf._merge's NMS step with equal scores pinned: its default, nms_gpu, sorts the already sorted segment once more with
    torch.argsort, which leaves equal scores in any order (and mirrored views do give equal scores); this is the same kernel on the
    segment as it stands, sorted by the stable rule of wbf.segment_order"""
    from cpd_amd import ops
    return ops.nms(torch.from_numpy(np.ascontiguousarray(boxes)).to(DEV), thresh).cpu().numpy()


def same(annos, want):
    assert len(annos) == len(want)
    for a, w in zip(annos, want):
        assert a["name"].tolist() == w["name"].tolist()
        assert a["score"].tobytes() == np.ascontiguousarray(w["score"], np.float32).tobytes()
        assert a["boxes_lidar"].tobytes() == np.ascontiguousarray(w["boxes_lidar"], np.float32).tobytes()


def end_to_end(T, engine, clouds, floors):
    merge = dict(RT.MERGE, WBF_PRE_SCORES=floors)
    augs = RT.augmentors(RT.INVERTIBLE)
    per_view, want = composition(engine, augs, clouds, merge, RT.CLASSES)
    print("boxes per (view, frame):", per_view, "merged:", [len(w["score"]) for w in want])
    assert min(per_view) >= 10, per_view                        # otherwise the comparison shows nothing
    assert all(len(w["score"]) > 0 for w in want)
    one = T.TTAEngine(engine, RT.INVERTIBLE, merge, RT.CLASSES)
    assert one.chunk >= len(clouds)
    res = one.forward(clouds)
    assert all(r["pred_boxes"].is_cuda for r in res)
    same(one.annos(res, range(len(clouds))), want)
    host = T.TTAEngine(engine, RT.INVERTIBLE, merge, RT.CLASSES, host_results=True).forward(clouds)
    for h, r in zip(host, res):
        assert not h["pred_boxes"].is_cuda and all(torch.equal(h[k], r[k].cpu()) for k in r)


def pipeline_clouds():
    from cpd_amd.synthetic import waymo_cloud
    out = []
    for seed, n in ((0, 60000), (1, 50000)):
        p = waymo_cloud(seed, n_points=n)
        p[:, :2] *= 0.3                                          # pull the scene into the crop
        out.append(torch.from_numpy(p).to(DEV))
    return out


def test_tta_engine_is_the_host_composition_centerpoint(T):
    import test_gpu_pipeline as P
    from cpd_amd.engine import CenterPointEngine, init_state_dict
    cfg = P.small_cfg()
    engine = CenterPointEngine(cfg, init_state_dict(cfg, seed=3))
    end_to_end(T, engine, pipeline_clouds(), [cfg.score_thresh, 0.0, cfg.score_thresh])


def test_tta_engine_is_the_host_composition_voxel_rcnn(T):
    import test_gpu_two_stage as P2
    engine = P2._model().to_engine()
    end_to_end(T, engine, pipeline_clouds(), [0.3, 0.0, 0.3])


def test_two_chunks_give_the_one_chunk_result(T):
    """max_batch = V: two chunks of one frame each give the detections of the one 2-frame chunk, bit for bit, when the range guard
    (which sees a whole engine batch) stays out of it. On the fp32 arithmetic: an engine step on the default split-fp16 arithmetic is
    itself not bit-invariant to the batch it runs in (the same frame alone and in a larger batch: scores 8e-7, boxes 1e-5 apart,
    measured on this config), which no chunking can undo; on fp32 it is."""
    import dataclasses
    import test_gpu_pipeline as P
    from cpd_amd.engine import CenterPointEngine, init_state_dict
    cfg = dataclasses.replace(P.small_cfg(), conv_math="f32")
    engine = CenterPointEngine(cfg, init_state_dict(cfg, seed=3))
    merge = dict(RT.MERGE, WBF_PRE_SCORES=[cfg.score_thresh, 0.0, cfg.score_thresh])
    clouds = pipeline_clouds()
    one = T.TTAEngine(engine, RT.INVERTIBLE, merge, RT.CLASSES)
    two = T.TTAEngine(engine, RT.INVERTIBLE, merge, RT.CLASSES, max_batch=len(RT.INVERTIBLE))
    assert one.chunk >= 2 and two.chunk == 1
    want = one.annos(one.forward(clouds), range(2))
    got = two.annos(two.forward(clouds), range(2))
    assert engine.range_reruns == 0 and engine.range_guarded_steps == 0
    assert min(len(w["score"]) for w in want) >= 10
    same(got, want)
