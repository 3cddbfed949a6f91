#!/usr/bin/env python3
"""Golden vectors of the test-time-augmentation fusion (tests/golden/wbf.npz). Only DATA is written.

What runs here is the reference's own text: DetectionsMerger.compute_WBF / merge_by_WBF / merge_by_NMS
(cpd/datasets/kitti/kitti_object_eval_python/merge_detections.py:93-228; the module itself does not import -- skimage, calibration,
a config file -- so the three methods' source is read from that file at maker time and executed on a stand-in class: the text is
never stored) and model_nms_utils.compute_WBF (cpd/models/model_utils/model_nms_utils.py:14-113, loaded by file path under the
synthetic package `r` of make_golden.py). Their iou3d_nms_utils.boxes_bev_iou_cpu is the compiled reference IoU of oracle/_ref
(oracle.binding.load_reference_iou), common_utils.limit_period is the reference's own, nms_gpu is the oracle's rotated NMS on host
tensors. The cluster each box ended in is read from the reference's own dictionaries when the method returns (a trace hook on its
frame), not derived.

Cases. Per evaluation-side case X (wbf_mean, wbf_pi, wbf_max, wbf_one): X_scores [n], X_boxes [n, 7] (floored and sorted: the
method's arguments), X_thresh, X_type, and the reference's X_out_scores, X_out_boxes, X_cluster_of [n], X_max_iou / X_second [n] (the
largest and the second largest IoU the method saw at every box; -1 where there was none). Per model case X (model_mean_retain,
model_max_retain, model_mean_noretain, model_max_noretain) the same plus X_thresh2, X_retain, X_n_single, X_branch [n] (0 join, 1
emitted, 2 dropped by l.65, 3 dropped by l.67, 4 opened, -1 the first box). merge_*: three frames of six views through
merge_by_WBF with MERGE_TYPE (WBF-mean, WBF-max, NMS): merge_names / merge_scores / merge_boxes with merge_n [3] in,
merge_out_* with merge_out_n [3] out; frame 1 has no Cyclist and one Pedestrian.

Asserted here (conditions of the exact GPU comparison, checked on the CPU; seeds are tried until they hold):
  at every step of every run |max_iou - t| >= 1e-3 for every threshold t the rule compares with (0.03 and iou_thresh2 included),
  whenever a box joins a cluster the runner-up IoU is at least 1e-3 below the maximum (the device IoU contract is 1e-4),
  every pair of the NMS class lies 1e-3 from NMS_IOU,
  wbf_mean holds a cluster of >= 4 members that differs from the textbook score-weighted mean of its original boxes by > 1e-4,
  wbf_pi holds a cluster whose members' folded headings straddle +-pi,
  the model cases together hold every one of the five branches, both retain_low values and both types.
Usage:  python tests/golden/make_golden_wbf.py
"""
import os
import re
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
import ref_wbf as R  # noqa: E402
from oracle import Oracle  # noqa: E402
from oracle.binding import load_reference_iou  # noqa: E402

REL = "cpd/datasets/kitti/kitti_object_eval_python/merge_detections.py"
CLASSES = ["Car", "Pedestrian", "Cyclist"]
MERGE_CFG = {"WBF_IOUS": [0.55, 0.3, 0.4], "WBF_PRE_SCORES": [0.1, 0.1, 0.1], "MERGE_TYPE": ["WBF-mean", "WBF-max", "NMS"], "NMS_IOU": 0.1}


class IouLog:
    """boxes_bev_iou_cpu of the compiled reference, remembering the two largest values of every call"""

    def __init__(self):
        self.fn = load_reference_iou()
        if self.fn is None:
            raise SystemExit("build oracle/_ref first: make -C oracle ref")
        self.calls = []

    def boxes_bev_iou_cpu(self, a, b):
        v = self.fn(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32))
        top = np.sort(v[0])[::-1]
        self.calls.append((float(top[0]), float(top[1]) if len(top) > 1 else -1.0))
        return v


def load_methods(log, oracle):
    iou_mod = types.ModuleType("r.ops.iou3d_nms.iou3d_nms_utils")
    iou_mod.boxes_bev_iou_cpu = log.boxes_bev_iou_cpu

    def nms_gpu(boxes, scores, thresh, **kw):
        order = np.argsort(-scores.numpy(), kind="stable")
        keep = oracle.nms(boxes.numpy()[order], thresh)
        return torch.from_numpy(order[keep]), None

    iou_mod.nms_gpu = nms_gpu
    torch.Tensor.cuda = lambda self, *a, **k: self               # merge_by_NMS moves its host arrays to the device
    for p in ["r", "r.utils", "r.ops", "r.ops.iou3d_nms", "r.models", "r.models.model_utils"]:
        MG._pkg(p)
    sys.modules["r.ops.iou3d_nms.iou3d_nms_utils"] = iou_mod
    sys.modules["r.ops.iou3d_nms"].iou3d_nms_utils = iou_mod
    common_utils = MG._load("r.utils.common_utils", "cpd/utils/common_utils.py")
    model_utils = MG._load("r.models.model_utils.model_nms_utils", "cpd/models/model_utils/model_nms_utils.py")
    text = open(os.path.join(MG.REF, REL)).read()
    ns = {"np": np, "torch": torch, "common_utils": common_utils, "iou3d_nms_utils": iou_mod}
    for name in ("merge_by_NMS", "compute_WBF", "merge_by_WBF"):
        m = re.search(r"^(    def %s\(.*?)(?=^    def )" % name, text, re.S | re.M)
        exec(textwrap.dedent(m.group(1)), ns)
    merger = type("Merger", (), {k: ns[k] for k in ("merge_by_NMS", "compute_WBF", "merge_by_WBF")})()
    merger.config = MG.AttrDict(MERGE_CFG)
    return merger, model_utils.compute_WBF


def run_traced(fn, *args, **kw):
    """fn(*args) -> (result, the locals of fn's own frame at its return)"""
    code = getattr(fn, "__func__", fn).__code__
    snap = {}

    def local(frame, event, arg):
        if event == "return":
            snap.update(frame.f_locals)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None

    sys.settrace(tracer)
    try:
        out = fn(*args, **kw)
    finally:
        sys.settrace(None)
    return out, snap


def clusters_of(snap, scores):
    """cluster_of [n] from the reference's cluster_score_dict (scores are distinct); boxes in no cluster: -9"""
    where = {float(s): i for i, s in enumerate(scores)}
    assert len(where) == len(scores), "scores are not distinct"
    out = np.full(len(scores), -9, np.int32)
    for k, members in snap["cluster_score_dict"].items():
        for s in members:
            out[where[float(s)]] = k
    return out


def per_box(log, n):
    a = np.full((n, 2), -1.0, np.float32)
    assert len(log.calls) == max(n - 1, 0)
    if n > 1:
        a[1:] = np.array(log.calls, np.float32)
    return a[:, 0], a[:, 1]


def check_margins(vmax, second, joined, thresholds):
    for i in range(1, len(vmax)):
        for t in thresholds:
            assert abs(float(vmax[i]) - float(np.float32(t))) >= 1e-3, "a max IoU within 1e-3 of %g" % t
        if joined[i]:
            assert float(vmax[i]) - float(second[i]) >= 1e-3, "a runner-up within 1e-3 of the maximum"


def run_wbf(merger, log, scores, boxes, thresh, kind):
    log.calls = []
    names = np.array(["Car"] * len(scores))
    (on, os_, ob), snap = run_traced(merger.compute_WBF, names, scores.copy(), boxes.copy(), thresh, kind)
    cl = clusters_of(snap, scores)
    assert (cl >= 0).all()
    vmax, second = per_box(log, len(scores))
    first = np.array([np.flatnonzero(cl == k)[0] for k in range(cl.max() + 1)])
    joined = np.ones(len(cl), bool)
    joined[first] = False
    check_margins(vmax, second, joined, [thresh])
    assert len(on) == len(os_) == len(ob) == cl.max() + 1
    return {"scores": scores, "boxes": boxes, "thresh": np.float64(thresh), "type": np.array(kind), "out_scores": np.asarray(os_, np.float32),
            "out_boxes": np.asarray(ob, np.float32).reshape(-1, 7), "cluster_of": cl, "max_iou": vmax, "second": second}


def run_model(model_fn, log, scores, boxes, thresh, thresh2, kind, retain):
    log.calls = []
    names = np.array(["Car"] * len(scores))
    (on, os_, ob), snap = run_traced(model_fn, names, scores.copy(), boxes.copy(), thresh, thresh2, kind, retain)
    cl = clusters_of(snap, scores)
    n_clusters = len(snap["cluster_score_dict"])
    n_single = len(os_) - n_clusters
    ob = np.asarray(ob, np.float32).reshape(-1, 7)
    for row in ob[:n_single]:                                    # the boxes emitted on their own are input rows (heading folded)
        hit = np.flatnonzero((boxes[:, :6] == row[:6]).all(1))
        assert len(hit) == 1 and cl[hit[0]] == -9
        cl[hit[0]] = R.SINGLE
    cl[cl == -9] = R.DROPPED
    vmax, second = per_box(log, len(scores))
    first = np.array([np.flatnonzero(cl == k)[0] for k in range(n_clusters)])
    joined = cl >= 0
    joined[first] = False
    check_margins(vmax, second, joined, [thresh, thresh2, 0.03])
    branch = np.full(len(cl), -1, np.int32)
    for i in range(1, len(cl)):
        if joined[i]:
            branch[i] = 0
        elif cl[i] == R.SINGLE:
            branch[i] = 1
        elif cl[i] == R.DROPPED:
            branch[i] = 2 if retain else 3
        else:
            branch[i] = 4
    return {"scores": scores, "boxes": boxes, "thresh": np.float64(thresh), "thresh2": np.float64(thresh2), "type": np.array(kind),
            "retain": np.array(retain), "out_scores": np.asarray(os_, np.float32), "out_boxes": ob, "cluster_of": cl,
            "n_single": np.int32(n_single), "max_iou": vmax, "second": second, "branch": branch}


def textbook_gap(case):
    """largest |reference - textbook score-weighted mean of the ORIGINAL boxes| over the clusters of >= 4 members"""
    gap = 0.0
    cl, s, b = case["cluster_of"], case["scores"].astype(np.float64), case["boxes"].astype(np.float64)
    for k in range(cl.max() + 1):
        m = np.flatnonzero(cl == k)
        if len(m) >= 4:
            gap = max(gap, np.abs((b[m, :6] * s[m, None]).sum(0) / s[m].sum() - case["out_boxes"][k, :6]).max())
    return gap


def straddles_pi(case):
    h = R.limit_period(case["boxes"][:, 6], 0.5, 2 * np.pi)
    cl = case["cluster_of"]
    return any((h[cl == k] > 3.0).any() and (h[cl == k] < -3.0).any() for k in range(cl.max() + 1))


def first_good(what, make):
    for seed in range(20261101, 20261101 + 400):
        try:
            got = make(np.random.default_rng(seed))
        except AssertionError as e:
            print("%s: seed %d rejected: %s" % (what, seed, e))
            continue
        print("%s: seed %d" % (what, seed))
        return got
    raise RuntimeError("%s: no seed meets the conditions" % what)


def main():
    oracle = Oracle()
    log = IouLog()
    merger, model_fn = load_methods(log, oracle)
    out = {}

    def put(name, case):
        for k, v in case.items():
            out["%s_%s" % (name, k)] = v

    def segment(rng, cls, **kw):
        names, scores, boxes = R.gen_detections(rng, classes=(cls,), **kw)
        return R.sorted_segment(scores, boxes, 0.05)

    def mean_case(rng):
        c = run_wbf(merger, log, *segment(rng, "Car", n_obj=10, views=(1, 6)), 0.55, "mean")
        assert textbook_gap(c) > 1e-4, "no cluster of >= 4 members away from the textbook mean"
        return c

    def pi_case(rng):
        c = run_wbf(merger, log, *segment(rng, "Car", n_obj=6, views=(3, 6), heading=np.pi, n_isolated=1, n_low=1), 0.55, "mean")
        assert straddles_pi(c), "no cluster straddles +-pi"
        return c

    put("wbf_mean", first_good("wbf_mean", mean_case))
    put("wbf_pi", first_good("wbf_pi", pi_case))
    put("wbf_max", first_good("wbf_max", lambda rng: run_wbf(merger, log, *segment(rng, "Pedestrian", n_obj=10, spacing=4.0), 0.3, "max")))
    put("wbf_one", first_good("wbf_one", lambda rng: run_wbf(merger, log, *segment(rng, "Cyclist", n_obj=0, n_isolated=1, n_low=1), 0.4, "mean")))
    assert len(out["wbf_one_scores"]) == 1

    def model_cases(rng):
        s, b = segment(rng, "Car", n_obj=14, views=(2, 6), jitter=2.0)
        cases = {"model_mean_retain": run_model(model_fn, log, s, b, 0.9, 0.5, "mean", True),
                 "model_max_retain": run_model(model_fn, log, s, b, 0.8, 0.4, "max", True),
                 "model_mean_noretain": run_model(model_fn, log, s, b, 0.85, 0.5, "mean", False),
                 "model_max_noretain": run_model(model_fn, log, s, b, 0.9, 0.5, "max", False)}
        seen = set(np.concatenate([c["branch"] for c in cases.values()]).tolist())
        assert {0, 1, 2, 3, 4} <= seen, "branches seen: %s" % sorted(seen)
        for c in cases.values():
            assert (c["branch"] == 0).any(), "a model case without a join"
        assert max(np.bincount(c["cluster_of"][c["cluster_of"] >= 0]).max() for c in cases.values()) >= 3
        return cases

    for name, case in first_good("model", model_cases).items():
        put(name, case)

    def merge_case(rng):
        frames = [R.gen_detections(rng, 9, views=(1, 6)), R.gen_detections(rng, 6, classes=("Car",), views=(1, 6), n_isolated=1, n_low=1),
                  R.gen_detections(rng, 8, views=(2, 6))]
        n1, s1, b1 = frames[1]
        n1 = n1.astype("<U10")
        n1[int(np.argmax(s1))] = "Pedestrian"                    # frame 1: one Pedestrian, no Cyclist
        frames[1] = (n1, s1, b1)
        res = []
        for names, scores, boxes in frames:
            names = names.astype("<U10")
            log.calls = []
            res.append(merger.merge_by_WBF(names.copy(), scores.copy(), boxes.copy()))
            for c, cls in enumerate(CLASSES):                    # the margins of every class's run, from the restatement's trace
                idx = R.class_segment(names, scores, cls, MERGE_CFG["WBF_PRE_SCORES"][c])
                if MERGE_CFG["MERGE_TYPE"][c] == "NMS":
                    v = log.fn(boxes[idx], boxes[idx]) if len(idx) else np.zeros((0, 0), np.float32)
                    assert v.size == 0 or np.abs(v - np.float32(MERGE_CFG["NMS_IOU"])).min() >= 1e-3, "an NMS pair within 1e-3 of NMS_IOU"
                else:
                    tr = R.compute_wbf(scores[idx], boxes[idx], MERGE_CFG["WBF_IOUS"][c], log.fn, MERGE_CFG["MERGE_TYPE"][c][4:])[3]
                    assert R.margins_ok(tr, [MERGE_CFG["WBF_IOUS"][c]]), "a merge segment without the margin"
        assert (frames[1][0] == "Cyclist").sum() == 0 and (frames[1][0] == "Pedestrian").sum() == 1
        assert all((r[0] == "Cyclist").any() for r in (res[0], res[2])), "no Cyclist through the NMS class"
        return frames, res

    frames, res = first_good("merge", merge_case)
    out["merge_names"] = np.concatenate([f[0].astype("<U10") for f in frames])
    out["merge_scores"] = np.concatenate([f[1] for f in frames])
    out["merge_boxes"] = np.concatenate([f[2] for f in frames])
    out["merge_n"] = np.array([len(f[1]) for f in frames], np.int32)
    out["merge_out_names"] = np.concatenate([np.asarray(r[0]).astype("<U10") for r in res])
    out["merge_out_scores"] = np.concatenate([np.asarray(r[1], np.float32) for r in res])
    out["merge_out_boxes"] = np.concatenate([np.asarray(r[2], np.float32).reshape(-1, 7) for r in res])
    out["merge_out_n"] = np.array([len(r[1]) for r in res], np.int32)
    for k in ("WBF_IOUS", "WBF_PRE_SCORES", "NMS_IOU"):
        out["merge_cfg_" + k] = np.array(MERGE_CFG[k], np.float64)
    out["merge_cfg_MERGE_TYPE"] = np.array(MERGE_CFG["MERGE_TYPE"])
    out["merge_classes"] = np.array(CLASSES)
    path = os.path.join(HERE, "wbf.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    for name in ("wbf_mean", "wbf_pi", "wbf_max", "wbf_one", "model_mean_retain", "model_max_retain", "model_mean_noretain", "model_max_noretain"):
        cl = out[name + "_cluster_of"]
        print(name, "boxes", len(cl), "out", len(out[name + "_out_scores"]), "largest cluster", np.bincount(cl[cl >= 0]).max())
    print("textbook gap", textbook_gap({k[9:]: v for k, v in out.items() if k.startswith("wbf_mean_")}))


if __name__ == "__main__":
    main()
