"""The rules of cpd_tta_collect on a machine without a GPU (cpd_tta_collect_cpu: csrc/tta_rules.h compiled for the host), against the
host path they replace: TestAugmentor.backward for the boxes, wbf.build_segment_table for which slots enter a segment and in what
order; and the argument limits of the two device entry points, which are checked before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import ref_tta as RT


@pytest.fixture(scope="module")
def T():
    from cpd_amd import tta
    return tta


def run_cpu(T, case, views, merge=RT.MERGE, classes=RT.CLASSES):
    seg = T.collect_cpu(*[torch.from_numpy(case[k].copy()) for k in ("boxes", "scores", "labels", "counts")], RT.augmentors(views), merge, classes,
                        case["batch"])
    return T.Segments(*[t.numpy() for t in seg])


@pytest.fixture(scope="module")
def backward_run(T):
    case = RT.backward_case()
    merge = dict(WBF_IOUS=[0.5], WBF_PRE_SCORES=[-1.0], MERGE_TYPE=["WBF-mean"], NMS_IOU=0.1)
    return case, run_cpu(T, case, RT.EIGHT, merge, RT.CLASSES[:1])


def test_backward_boxes_are_test_augmentor_backward(backward_run):
    case, seg = backward_run
    n_views, cap = case["n_views"], case["cap"]
    assert seg.count.tolist() == [n_views * cap] and seg.start.tolist() == [0]
    src = seg.src[0]
    assert sorted(src.tolist()) == list(range(n_views * cap))                    # every slot once ...
    flat_scores = case["scores"].reshape(-1)
    assert np.array_equal(src, np.argsort(-flat_scores, kind="stable"))           # ... by descending score
    assert seg.scores[0].tobytes() == flat_scores[src].tobytes()
    want = RT.host_backward(RT.augmentors(RT.EIGHT), case["boxes"], case["counts"], 1)
    for v in range(n_views):
        rows = np.flatnonzero(src // cap == v)
        RT.check_backward(seg.boxes[0][rows], want[v][src[rows] % cap], case["boxes"][v][src[rows] % cap], RT.ROTATED[v], "view %d" % v)
    assert RT.ROTATED == [False, True, True, False, True, True, False, False]


def test_backward_boxes_of_the_reference_golden(T, golden):
    z = golden("augment")
    table = np.ascontiguousarray(z["view_boxes_in"], np.float32)
    n = len(table)
    case = dict(boxes=np.ascontiguousarray(np.broadcast_to(table, (6, n, 7))), scores=np.broadcast_to(np.linspace(1, 0.5, n, dtype=np.float32), (6, n)).copy(),
                labels=np.ones((6, n), np.int64), counts=np.full((6,), n, np.int32), batch=1)
    merge = dict(WBF_IOUS=[0.5], WBF_PRE_SCORES=[0.0], MERGE_TYPE=["WBF-max"], NMS_IOU=0.1)
    seg = run_cpu(T, case, RT.SHIPPED, merge, RT.CLASSES[:1])
    assert seg.count.tolist() == [6 * n]
    # equal scores across the views: the views alternate, each row's six copies in view order
    assert np.array_equal(seg.src[0], (np.arange(6)[None, :] * n + np.arange(n)[:, None]).reshape(-1))
    for v in range(6):
        RT.check_backward(seg.boxes[0][v::6], z["view%d_back" % v], table, RT.ROTATED[v], "golden view %d" % v)


@pytest.fixture(scope="module")
def segment_run(T):
    case = RT.segment_case()
    return case, run_cpu(T, case, RT.EIGHT)


def test_segments_are_build_segment_table(T, segment_run):
    from cpd_amd import wbf
    case, seg = segment_run
    n_views, cap, batch, n_class = case["n_views"], case["cap"], case["batch"], len(RT.CLASSES)
    vk = n_views * cap
    frames = RT.frame_lists(RT.label_names(case["labels"]), case["scores"], case["boxes"], case["counts"], n_views, batch)
    # frames 0 .. 2 through build_segment_table (frame 3 holds the segment it refuses)
    table = wbf.build_segment_table([(n, s) for n, s, _, _ in frames[:3]], RT.MERGE, RT.CLASSES)
    slot = np.concatenate([f[3] for f in frames[:3]])
    assert seg.start.tolist() == [s * vk for s in range(batch * n_class)]
    assert seg.count[:3 * n_class].tolist() == table.count.tolist()
    assert seg.mode.tolist() == table.mode.tolist() + table.mode[:n_class].tolist()
    assert seg.thresh.tobytes() == np.concatenate([table.thresh, table.thresh[:n_class]]).tobytes()
    all_scores = np.concatenate([f[1] for f in frames[:3]])
    for s in range(3 * n_class):
        a, c = int(table.start[s]), int(table.count[s])
        assert np.array_equal(seg.src[s, :c], slot[table.order[a:a + c]]), "segment %d" % s
        assert seg.scores[s, :c].tobytes() == all_scores[table.order[a:a + c]].tobytes()
        assert (seg.src[s, c:] == -1).all()
    nms = np.array(RT.MERGE["MERGE_TYPE"] * batch) == "NMS"
    assert np.array_equal(seg.count_wbf, np.where(nms, 0, seg.count)) and np.array_equal(seg.count_nms, np.where(nms & (seg.count > 0), seg.count, 0))
    # what the case is there for
    assert seg.count[n_class:2 * n_class].tolist() == [0, 0, 0]                                  # the frame with no box at all
    assert seg.count[2 * n_class] == RT.MAX_SEGMENT == wbf.MAX_SEGMENT                            # exactly the limit: accepted
    for c in range(n_class):
        kept = set(seg.src[c, :seg.count[c]].tolist())
        for v in (5, 6):
            at, below = case["special"][(c, v)]
            assert at in kept and below not in kept                                              # at the floor: kept; one step below: dropped
    s0 = seg.scores[0, :seg.count[0]]
    ties = np.flatnonzero(s0[1:] == s0[:-1])
    views_of = seg.src[0, :seg.count[0]] // cap
    assert (views_of[ties] == views_of[ties + 1]).any() and (views_of[ties] != views_of[ties + 1]).any()   # ties within and across views
    assert (np.diff(seg.src[0, :seg.count[0]])[ties] > 0).all()
    assert sorted(set(case["counts"].reshape(n_views, batch)[:, 0].tolist())) == [0, 1, 37, 63, 64, 65, 200, 300]
    # frame 3: class 0 is one over the limit and refused, the other classes as segment_order has them
    assert seg.count[3 * n_class] == -1 and seg.count_wbf[3 * n_class] == -1 and seg.count_nms[3 * n_class] == 0
    assert (seg.src[3 * n_class] == -1).all()
    names, scores, _, slots = frames[3]
    assert ((names == RT.CLASSES[0]) & (scores >= np.float32(RT.MERGE["WBF_PRE_SCORES"][0]))).sum() == RT.MAX_SEGMENT + 1
    for c in (1, 2):
        order = wbf.segment_order(names, scores, RT.CLASSES[c], RT.MERGE["WBF_PRE_SCORES"][c])
        assert seg.count[3 * n_class + c] == len(order) > 0
        assert np.array_equal(seg.src[3 * n_class + c, :len(order)], slots[order])
    with pytest.raises(ValueError, match="refused a segment"):
        T.check_segments(seg.count.tolist())
    T.check_segments(seg.count[:3 * n_class].tolist())
    with pytest.raises(ValueError):
        wbf.build_segment_table([(names, scores)], RT.MERGE, RT.CLASSES)


def test_segment_boxes_follow_their_slots(T, segment_run):
    case, seg = segment_run
    n_views, cap, batch = case["n_views"], case["cap"], case["batch"]
    want = RT.host_backward(RT.augmentors(RT.EIGHT), case["boxes"], case["counts"], batch)
    for s in range(len(seg.count)):
        f, c = s // len(RT.CLASSES), max(int(seg.count[s]), 0)
        src = seg.src[s, :c]
        for v in range(n_views):
            rows = np.flatnonzero(src // cap == v)
            blk = v * batch + f
            RT.check_backward(seg.boxes[s][rows], want[blk][src[rows] % cap], case["boxes"][blk][src[rows] % cap], RT.ROTATED[v], (s, v))


def test_limits_are_error_codes(T):
    from cpd_amd import _lib
    lib = _lib.lib()
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)

    def views(n_views, n_total, n_ops):
        kind, param = np.zeros((n_views, T.MAX_OPS), np.int32), np.zeros((n_views, T.MAX_OPS, 2))
        n = np.full((n_views,), n_ops, np.int32)
        off = np.array([0, n_total], np.int64)
        return lib.cpd_tta_views(None, n_total, 4, vp(off), 1, vp(kind), vp(param), vp(n), n_views, None, None)
    assert views(16, 0, 8) == 0                                     # at the limits (no point: nothing is launched)
    assert views(17, 0, 1) == -1
    assert views(16, 0, 9) == -1
    assert views(8, 2 ** 28, 1) == -1                               # V * N_total = 2^31
    case = RT.backward_case()
    boxes, scores, labels, counts = [torch.from_numpy(case[k].copy()) for k in ("boxes", "scores", "labels", "counts")]
    augs = RT.augmentors(RT.EIGHT)
    merge = dict(WBF_IOUS=[0.5] * 17, WBF_PRE_SCORES=[0.0] * 17, MERGE_TYPE=["WBF-mean"] * 17, NMS_IOU=0.1)
    with pytest.raises(_lib.CpdHipError, match="CPD_ERR_ARG"):
        T.collect_cpu(boxes, scores, labels, counts, augs, merge, ["c%d" % i for i in range(17)], 1)
    long_view = RT.augmentors([RT.view_cfg(axis="x") * 3])          # nine ops
    with pytest.raises(_lib.CpdHipError, match="CPD_ERR_ARG"):
        T.collect_cpu(boxes[:1], scores[:1], labels[:1], counts[:1], long_view, merge, ["c0"], 1)


def test_annos_and_op_lists(T):
    augs = RT.augmentors([RT.view_cfg(RT.ROT, "x", 0.95)])
    fwd, back = T.view_ops(augs[0]), T.back_ops(augs[0])
    assert [o[0] for o in fwd] == [T.ROT, T.FLIP_X, T.SCALE] and [o[0] for o in back] == [T.SCALE, T.FLIP_X, T.ROT]
    assert back[2][3] == -RT.ROT and back[0][1] == 0.95
    eng = T.TTAEngine.__new__(T.TTAEngine)
    eng.class_names = list(RT.CLASSES)
    res = [dict(pred_boxes=torch.zeros((2, 7)), pred_scores=torch.tensor([0.5, 0.25]), pred_labels=torch.tensor([3, 1])),
           dict(pred_boxes=torch.zeros((0, 7)), pred_scores=torch.zeros((0,)), pred_labels=torch.zeros((0,), dtype=torch.int64))]
    annos = eng.annos(res, ["a", "b"])
    assert annos[0]["name"].tolist() == [RT.CLASSES[2], RT.CLASSES[0]] and annos[0]["frame_id"] == "a"
    assert annos[1]["boxes_lidar"].shape == (0, 7) and len(annos[1]["name"]) == 0
