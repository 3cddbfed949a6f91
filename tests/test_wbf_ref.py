"""CPU: the restatement of the test-time-augmentation fusion (tests/ref_wbf.py) against the reference's own methods
(tests/golden/wbf.npz, made by tests/golden/make_golden_wbf.py), and the host side of cpd_amd.wbf (segment table, merge_by_WBF /
merge_frames with the restatement injected in place of the launch, the size limit) with no kernel involved."""
import os
import re

import numpy as np
import pytest

import ref_wbf as R

WBF_CASES = ("wbf_mean", "wbf_pi", "wbf_max", "wbf_one")
MODEL_CASES = ("model_mean_retain", "model_max_retain", "model_mean_noretain", "model_max_noretain")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wz(golden):
    return golden("wbf")


def merge_cfg(wz):
    return {"WBF_IOUS": list(wz["merge_cfg_WBF_IOUS"]), "WBF_PRE_SCORES": list(wz["merge_cfg_WBF_PRE_SCORES"]),
            "MERGE_TYPE": [str(t) for t in wz["merge_cfg_MERGE_TYPE"]], "NMS_IOU": float(wz["merge_cfg_NMS_IOU"])}


def merge_frames_in(wz, prefix="merge_"):
    cut = np.cumsum([0] + list(wz[prefix + "n"]))
    return [(wz[prefix + "names"][a:b], wz[prefix + "scores"][a:b], wz[prefix + "boxes"][a:b]) for a, b in zip(cut[:-1], cut[1:])]


def run_case(wz, oracle, name):
    s, b = wz[name + "_scores"], wz[name + "_boxes"]
    kind = str(wz[name + "_type"])
    if name.startswith("model"):
        return R.model_compute_wbf(s, b, oracle.boxes_iou_bev, float(wz[name + "_thresh"]), float(wz[name + "_thresh2"]), kind,
                                   bool(wz[name + "_retain"]))
    return R.compute_wbf(s, b, float(wz[name + "_thresh"]), oracle.boxes_iou_bev, kind)


@pytest.mark.parametrize("name", WBF_CASES + MODEL_CASES)
def test_restatement_matches_the_reference_method(wz, oracle, name):
    got = run_case(wz, oracle, name)
    assert np.array_equal(got[2], wz[name + "_cluster_of"])                       # the cluster of every box, and with it the order
    assert np.array_equal(got[0], wz[name + "_out_scores"])                       # the same numpy arithmetic on both sides
    assert np.array_equal(got[1], wz[name + "_out_boxes"])
    if name.startswith("model"):
        assert got[4] == wz[name + "_n_single"]
    thresholds = [wz[name + "_thresh"]] + ([wz[name + "_thresh2"], 0.03] if name.startswith("model") else [])
    assert R.margins_ok(got[3], thresholds)
    vmax = np.array([-1.0] + [t[1] for t in got[3]], np.float32)
    assert np.abs(vmax - wz[name + "_max_iou"]).max() <= 1e-6                     # oracle IoU against the compiled reference's


def test_golden_covers_the_quirks(wz):
    cl, s, b = wz["wbf_mean_cluster_of"], wz["wbf_mean_scores"].astype(np.float64), wz["wbf_mean_boxes"].astype(np.float64)
    gap = 0.0
    for k in range(cl.max() + 1):                                                 # the aliasing quirk: not the textbook weighted mean
        m = np.flatnonzero(cl == k)
        if len(m) >= 4:
            gap = max(gap, np.abs((b[m, :6] * s[m, None]).sum(0) / s[m].sum() - wz["wbf_mean_out_boxes"][k, :6]).max())
    assert gap > 1e-4
    h, cl = R.limit_period(wz["wbf_pi_boxes"][:, 6], 0.5, 2 * np.pi), wz["wbf_pi_cluster_of"]
    assert any((h[cl == k] > 3.0).any() and (h[cl == k] < -3.0).any() for k in range(cl.max() + 1))
    seen = set(np.concatenate([wz[n + "_branch"] for n in MODEL_CASES]).tolist())
    assert {0, 1, 2, 3, 4} <= seen
    assert {bool(wz[n + "_retain"]) for n in MODEL_CASES} == {True, False}
    assert {str(wz[n + "_type"]) for n in MODEL_CASES} == {"mean", "max"}
    for n in WBF_CASES + MODEL_CASES:                                             # distinct scores, descending: the sort is not in doubt
        assert (np.diff(wz[n + "_scores"]) < 0).all()
        thresholds = [wz[n + "_thresh"]] + ([wz[n + "_thresh2"], 0.03] if n.startswith("model") else [])
        for t in thresholds:
            assert np.abs(wz[n + "_max_iou"][1:] - np.float32(t)).min(initial=1.0) >= 1e-3
    f1 = merge_frames_in(wz)[1][0]
    assert (f1 == "Cyclist").sum() == 0 and (f1 == "Pedestrian").sum() == 1 and (f1 == "Car").sum() > 1
    assert all(len(np.unique(s)) == len(s) for _, s, _ in merge_frames_in(wz))    # distinct within a frame: the sort is not in doubt


def test_pairwise_mean_is_numpys():
    """A self-check of the restatement alone (it touches nothing of cpd_amd and passes without the feature): np_mean_f32 spells
    out numpy's pairwise sum so that the kernel's copy in csrc/wbf_rules.h has a text to be read against."""
    rng = np.random.default_rng(3)
    for n in list(range(0, 20)) + [63, 64, 65, 127, 128, 129, 136, 255, 256, 257, 1000, 1031]:
        a = (rng.normal(0, 1, n) * 10 ** rng.uniform(-3, 1)).astype(np.float32)
        want = a.mean() if n else np.float32(np.nan)
        assert np.array_equal(R.np_mean_f32(a), want, equal_nan=True), n


def test_limit_folds():
    """A self-check of the restatement alone, like the one above: both heading folds land in their interval and keep the angle."""
    a = np.array([0.0, 3.2, -3.2, 6.3, -6.3, 9.5, -0.1, np.pi, -np.pi], np.float32)
    lim = R.limit(a)
    assert (lim <= np.float32(np.pi)).all() and (lim >= np.float32(-np.pi)).all()
    assert np.abs(np.exp(1j * lim.astype(np.float64)) - np.exp(1j * a.astype(np.float64))).max() < 1e-5
    lp = R.limit_period(a, 0.5, 2 * np.pi)
    assert (lp < np.pi + 1e-6).all() and (lp >= -np.pi - 1e-6).all()


def test_segment_table_by_hand():
    from cpd_amd import wbf
    cfg = {"WBF_IOUS": [0.55, 0.3, 0.4], "WBF_PRE_SCORES": [0.5, 0.2, 0.1], "MERGE_TYPE": ["WBF-mean", "NMS", "WBF-max"], "NMS_IOU": 0.1}
    classes = ("Car", "Pedestrian", "Cyclist")
    f0 = (np.array(["Car", "Cyclist", "Car", "Pedestrian", "Car", "Car", "Truck"]), np.array([0.6, 0.3, 0.5, 0.25, 0.49, 0.9, 0.99], np.float32))
    f1 = (np.array(["Cyclist", "Cyclist", "Cyclist"]), np.array([0.2, 0.05, 0.7], np.float32))
    t = wbf.build_segment_table([f0, f1], cfg, classes)
    # frame 0: Car floor 0.5 (>=: 0.5 stays, 0.49 goes) sorted 0.9, 0.6, 0.5; Pedestrian; Cyclist. frame 1 (rows from 7): no Car, no
    # Pedestrian, Cyclist 0.7, 0.2 (0.05 below the floor). Unknown classes belong to no segment.
    assert t.order.tolist() == [5, 0, 2, 3, 1, 9, 7]
    assert t.start.tolist() == [0, 3, 4, 5, 5, 5] and t.count.tolist() == [3, 1, 1, 0, 0, 2]
    assert t.mode.tolist() == [wbf.MODE_MEAN, wbf.MODE_NMS, wbf.MODE_MAX] * 2
    assert t.frame.tolist() == [0, 0, 0, 1, 1, 1] and t.cls.tolist() == [0, 1, 2, 0, 1, 2]
    assert np.allclose(t.thresh, [[0.55, 0], [0.3, 0], [0.4, 0]] * 2)
    tie = wbf.build_segment_table([(np.array(["Car"] * 4), np.array([0.7, 0.9, 0.7, 0.9], np.float32))], cfg, ("Car",))
    assert tie.order.tolist() == [1, 3, 0, 2]                                     # ties: ascending original index
    empty = wbf.build_segment_table([], cfg, classes)
    assert empty.order.size == 0 and empty.start.size == 0


def test_views_are_concatenated_in_order(wz, oracle):
    from cpd_amd import wbf
    frames = merge_frames_in(wz)
    cfg, classes = merge_cfg(wz), tuple(str(c) for c in wz["merge_classes"])
    views = []
    for v in range(3):                                                            # three views: every third box of each frame
        views.append([{"name": n[v::3], "score": s[v::3], "boxes_lidar": b[v::3], "frame_id": "f%d" % f, "view": v}
                      for f, (n, s, b) in enumerate(frames)])
    seen = []

    def cluster(boxes, scores, start, count, thresh, mode):
        seen.append((boxes.copy(), scores.copy(), start.copy(), count.copy()))
        return R.make_cluster(oracle.boxes_iou_bev)(boxes, scores, start, count, thresh, mode)

    def nms(boxes, scores, thresh):
        return oracle.nms(boxes, thresh)

    out = wbf.merge_frames(views, cfg, classes, _cluster=cluster, _nms=nms)
    assert len(seen) == 1                                                         # one launch for all frames
    cat = [tuple(np.concatenate([a[v::3] for v in range(3)]) for a in fr) for fr in frames]
    want = wbf.build_segment_table([(n, s) for n, s, _ in cat], cfg, classes)
    assert np.array_equal(seen[0][1], np.concatenate([c[1] for c in cat])[want.order])
    wbf_rows = want.mode != wbf.MODE_NMS
    assert np.array_equal(seen[0][2], want.start[wbf_rows]) and np.array_equal(seen[0][3], want.count[wbf_rows])
    for f, (n, s, b) in enumerate(cat):                                           # the fused frame = merge_by_WBF of the concatenation
        en, es, eb = R.merge_by_wbf(n, s, b, cfg, oracle.boxes_iou_bev, oracle.nms, classes)
        assert np.array_equal(out[f]["name"], en) and np.array_equal(out[f]["score"], es) and np.array_equal(out[f]["boxes_lidar"], eb)
        assert out[f]["frame_id"] == "f%d" % f and out[f]["view"] == 0
    assert views[0][0]["name"].shape == frames[0][0][0::3].shape                  # view 0's own list is untouched (a deep copy)


def test_merge_by_wbf_reproduces_the_reference(wz, oracle):
    from cpd_amd import wbf
    cfg, classes = merge_cfg(wz), tuple(str(c) for c in wz["merge_classes"])
    assert "NMS" in cfg["MERGE_TYPE"] and "WBF-mean" in cfg["MERGE_TYPE"] and "WBF-max" in cfg["MERGE_TYPE"]
    cluster = R.make_cluster(oracle.boxes_iou_bev)
    cut = np.cumsum([0] + list(wz["merge_out_n"]))
    frames = merge_frames_in(wz)
    for f, (n, s, b) in enumerate(frames):
        keep = (n.copy(), s.copy(), b.copy())
        gn, gs, gb = wbf.merge_by_WBF(n, s, b, cfg, classes, _cluster=cluster, _nms=lambda bx, sc, t: oracle.nms(bx, t))
        a, e = cut[f], cut[f + 1]
        assert np.array_equal(gn, wz["merge_out_names"][a:e])
        assert np.array_equal(gs, wz["merge_out_scores"][a:e]) and gs.dtype == np.float32
        assert np.array_equal(gb, wz["merge_out_boxes"][a:e]) and gb.dtype == np.float32
        assert all(np.array_equal(x, y) for x, y in zip(keep, (n, s, b)))          # the documented deviation: inputs stay as they were
        rn, rs, rb = R.merge_by_wbf(n, s, b, cfg, oracle.boxes_iou_bev, oracle.nms, classes)
        assert np.array_equal(rn, gn) and np.array_equal(rs, gs) and np.array_equal(rb, gb)
    views = [[{"name": n, "score": s, "boxes_lidar": b} for n, s, b in frames]]
    out = wbf.merge_frames(views, cfg, classes, _cluster=cluster, _nms=lambda bx, sc, t: oracle.nms(bx, t))
    assert np.array_equal(np.concatenate([o["boxes_lidar"] for o in out]), wz["merge_out_boxes"])
    assert np.array_equal(np.concatenate([o["score"] for o in out]), wz["merge_out_scores"])


@pytest.mark.parametrize("name", WBF_CASES + MODEL_CASES)
def test_public_functions_with_the_restatement_injected(wz, oracle, name):
    from cpd_amd import wbf
    s, b = wz[name + "_scores"], wz[name + "_boxes"]
    names = np.array(["n%d" % i for i in range(len(s))])
    cluster = R.make_cluster(oracle.boxes_iou_bev)
    if name.startswith("model"):
        gn, gs, gb = wbf.model_compute_WBF(names, s, b, float(wz[name + "_thresh"]), float(wz[name + "_thresh2"]), str(wz[name + "_type"]),
                                           bool(wz[name + "_retain"]), _cluster=cluster)
        cl = wz[name + "_cluster_of"]
        first = [np.flatnonzero(cl == k)[0] for k in range(cl.max() + 1)]
        assert gn.tolist() == names[cl == R.SINGLE].tolist() + names[first].tolist()      # l.64, l.103 / l.107
    else:
        gn, gs, gb = wbf.compute_WBF(names, s, b, float(wz[name + "_thresh"]), str(wz[name + "_type"]), _cluster=cluster)
        assert gn.tolist() == names[:len(gs)].tolist()                                     # l.179
    assert np.array_equal(gs, wz[name + "_out_scores"]) and np.array_equal(gb, wz[name + "_out_boxes"])


def test_frames_without_boxes(oracle):
    from cpd_amd import wbf
    cfg = {"WBF_IOUS": [0.5, 0.5, 0.5], "WBF_PRE_SCORES": [0.1] * 3, "MERGE_TYPE": ["WBF-mean", "WBF-max", "NMS"], "NMS_IOU": 0.1}
    none = {"name": np.zeros(0, "<U3"), "score": np.zeros(0, np.float32), "boxes_lidar": np.zeros((0, 7), np.float32)}
    names, scores, boxes = R.gen_detections(np.random.default_rng(5), 4)
    some = {"name": names, "score": scores, "boxes_lidar": boxes}
    hooks = dict(_cluster=R.make_cluster(oracle.boxes_iou_bev), _nms=lambda b, s, t: oracle.nms(b, t))
    out = wbf.merge_frames([[none, some, none], [none, none, none]], cfg, **hooks)
    assert [len(o["score"]) for o in out][::2] == [0, 0] and out[0]["boxes_lidar"].shape == (0, 7)
    want = wbf.merge_by_WBF(names, scores, boxes, cfg, **hooks)
    assert len(want[1]) > 0 and all(np.array_equal(out[1][k], w) for k, w in zip(("name", "score", "boxes_lidar"), want))
    attr = type("Cfg", (), cfg)()                                                 # an attribute object serves as well as a dict
    assert all(np.array_equal(a, b) for a, b in zip(wbf.merge_by_WBF(names, scores, boxes, attr, **hooks), want))


@pytest.mark.parametrize("name", WBF_CASES + MODEL_CASES)
def test_host_build_of_the_rules_reproduces_the_reference(wz, name):
    """csrc/wbf_rules.h compiled for the host (cpd_wbf_cluster_cpu): the text the kernel runs, held to the reference's own results
    with no device involved -- clusters, order, boxes and scores bit for bit"""
    from cpd_amd import wbf
    s, b = wz[name + "_scores"], wz[name + "_boxes"]
    model = name.startswith("model")
    mode = (wbf.MODE_MAX if str(wz[name + "_type"]) == "max" else wbf.MODE_MEAN) | (wbf.MODE_MODEL if model else 0)
    if model and not bool(wz[name + "_retain"]):
        mode |= wbf.MODE_NO_RETAIN
    thresh = np.array([[wz[name + "_thresh"], wz[name + "_thresh2"] if model else 0.0]], np.float32)
    pad = np.full((2, 7), 3.0, np.float32)                                        # two rows before the segment that nobody owns
    ob, os_, oc, cl = wbf.cluster_segments_host(np.concatenate([pad, b]), np.concatenate([np.ones(2, np.float32), s]),
                                                np.array([2], np.int32), np.array([len(s)], np.int32), thresh, np.array([mode], np.int32))
    k = len(wz[name + "_out_scores"])
    assert oc.tolist() == [k] and np.array_equal(cl[2:], wz[name + "_cluster_of"]) and (cl[:2] == -3).all()
    assert np.array_equal(os_[2:2 + k], wz[name + "_out_scores"]) and np.array_equal(ob[2:2 + k], wz[name + "_out_boxes"])
    assert not ob[:2].any() and not ob[2 + k:].any()
    fn, args = ((wbf.model_compute_WBF, (float(thresh[0, 0]), float(thresh[0, 1]), str(wz[name + "_type"]), bool(wz[name + "_retain"])))
                if model else (wbf.compute_WBF, (float(thresh[0, 0]), str(wz[name + "_type"]))))
    gn, gs, gb = fn(np.arange(len(s)), s, b, *args, _cluster=wbf.cluster_segments_host)
    assert np.array_equal(gs, wz[name + "_out_scores"]) and np.array_equal(gb, wz[name + "_out_boxes"])


def test_host_build_of_the_rules_on_generated_segments(oracle):
    """every mode on generated segments that keep the margins, a 40-member WBF-mean chain, and model clusters of 9, 130 and 300
    members (the three paths of the pairwise heading mean): the host build equals the restatement bit for bit"""
    from cpd_amd import wbf
    iou = oracle.boxes_iou_bev
    modes = [(0, 0.55, 0.0), (1, 0.7, 0.0), (2, 0.9, 0.5), (3, 0.8, 0.4), (6, 0.85, 0.5), (7, 0.9, 0.5)]
    segs = []
    for seed in range(6):
        rng = np.random.default_rng(seed)
        _, sc, bx = R.gen_detections(rng, 10, classes=("Car",), jitter=[0.5, 1, 2, 4][seed % 4])
        segs += [(R.sorted_segment(sc, bx, 0.05), m) for m in modes]
    base = np.array([3.0, -2.0, 0.3, 4.7, 2.1, 1.7, 3.1])
    for n, m, rel in ((40, (0, 0.3, 0.0), 0.15), (9, (2, 0.9, 0.5), 0.004), (130, (2, 0.9, 0.5), 0.004), (300, (6, 0.9, 0.5), 0.004)):
        rng = np.random.default_rng(n)
        bx = np.tile(base, (n, 1))
        bx[:, :2] += rng.normal(0, rel, (n, 2))
        bx[:, 6] += rng.normal(0, rel * 2, n)
        segs.append(((np.sort(rng.uniform(0.1, 0.95, n))[::-1].astype(np.float32), bx.astype(np.float32)), m))
    checked = 0
    for (sc, bx), (mode, thr, thr2) in segs:
        kind = "max" if mode & 1 else "mean"
        if mode & 2:
            rs, rb, rc, tr = R.model_compute_wbf(sc, bx, iou, thr, thr2, kind, not (mode & 4))[:4]
        else:
            rs, rb, rc, tr = R.compute_wbf(sc, bx, thr, iou, kind)
        if not R.margins_ok(tr, [thr, thr2, 0.03] if mode & 2 else [thr], 1e-4):   # (host IoU against the oracle's: both within 1e-6 of the reference)
            continue
        ob, os_, oc, cl = wbf.cluster_segments_host(bx, sc, np.zeros(1, np.int32), np.array([len(sc)], np.int32),
                                                    np.array([[thr, thr2]], np.float32), np.array([mode], np.int32))
        assert oc[0] == len(rs) and np.array_equal(cl, rc)
        assert np.array_equal(os_[:oc[0]], rs, equal_nan=True) and np.array_equal(ob[:oc[0]], rb, equal_nan=True)
        checked += 1
    assert checked >= 30 and len(segs) == 40


def test_no_frames_and_no_views_of_a_frame():
    from cpd_amd import wbf
    cfg = {"WBF_IOUS": [0.5], "WBF_PRE_SCORES": [0.1], "MERGE_TYPE": ["WBF-mean"], "NMS_IOU": 0.1}
    assert wbf.merge_frames([[], []], cfg, ("Car",)) == []                        # views of an empty split: nothing to launch


def test_oversized_segment_raises():
    from cpd_amd import wbf
    n = wbf.MAX_SEGMENT + 1
    names, scores, boxes = np.array(["Car"] * n), np.linspace(0.9, 0.2, n).astype(np.float32), np.zeros((n, 7), np.float32)
    cfg = {"WBF_IOUS": [0.5], "WBF_PRE_SCORES": [0.1], "MERGE_TYPE": ["WBF-mean"], "NMS_IOU": 0.1}

    def never(*a):
        raise AssertionError("launched")

    with pytest.raises(ValueError):
        wbf.compute_WBF(names, scores, boxes, 0.5, _cluster=never)
    with pytest.raises(ValueError):
        wbf.model_compute_WBF(names, scores, boxes, _cluster=never)
    with pytest.raises(ValueError):
        wbf.merge_by_WBF(names, scores, boxes, cfg, ("Car",), _cluster=never)
    with pytest.raises(ValueError):                                               # the entry point itself refuses it whole
        wbf.cluster_segments_host(boxes, scores, np.zeros(1, np.int32), np.array([n], np.int32), np.array([[0.5, 0]], np.float32),
                                  np.zeros(1, np.int32))
    cfg["MERGE_TYPE"] = ["NMS"]                                                   # the NMS path has no such limit
    t = wbf.build_segment_table([(names, scores)], cfg, ("Car",))
    assert t.count.tolist() == [n]
    e = np.zeros(0)
    assert wbf.compute_WBF(e, e, e.reshape(0, 7), 0.5, _cluster=never)[0] is e    # l.111-112: empty in, the arguments out


def test_constants_match_the_header():
    from cpd_amd import wbf
    txt = open(os.path.join(REPO, "include", "cpd_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (CPD_WBF_[A-Z_]+) (\d+)", txt)}
    assert (val["CPD_WBF_MAX"], val["CPD_WBF_MODEL"], val["CPD_WBF_NO_RETAIN"]) == (wbf.MODE_MAX, wbf.MODE_MODEL, wbf.MODE_NO_RETAIN)
    assert (val["CPD_WBF_MAX_SEGMENT"], val["CPD_WBF_LDS_CLUSTERS"], val["CPD_WBF_BLOCK"]) == (wbf.MAX_SEGMENT, wbf.LDS_CLUSTERS, wbf.BLOCK)
    assert wbf.MAX_SEGMENT >= 4096 and (wbf.DROPPED, wbf.SINGLE) == (R.DROPPED, R.SINGLE)
