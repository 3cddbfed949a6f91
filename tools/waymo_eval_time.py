#!/usr/bin/env python3
"""Time cpd_amd.waymo_eval / cpd_amd.waymo_eval2d on a synthetic Waymo-format split (cpd_amd.synthetic.waymo_infos: 2000
frames, about 150 predictions and 60 ground truths per frame, mixed types). Prints one JSON line: the whole evaluation by
the host clock (median of --reps calls after one warm-up), the launches (cpd_waymo_iou or cpd_waymo_iou_bev once,
cpd_waymo_match once per threshold set) from HIP events over the prepared arrays of the whole split (median of --event-reps
passes after one warm-up pass), and the numpy / scipy restatement (tests/ref_waymo_eval.py, tests/ref_waymo_eval2d.py) on
one core of the same host on a --ref-frames subset. --protocol 3d is waymo_eval.py's (TYPE_3D, 0.7 / 0.5 / 0.5 / 0.5), 2d is
waymo_eval2d.py's (TYPE_2D, 0.5 / 0.3 / 0.3 / 0.3). --threshold-sets N evaluates N sets in one call (the protocol's own,
then its vehicle threshold lowered by 0.1 a set) through waymo_evaluation_at; the restatement is skipped then.
Not part of bench.py.
Usage: python tools/waymo_eval_time.py [--protocol 3d|2d] [--threshold-sets 1] [--frames 2000] [--reps 3] [--ref-frames 100]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import _lib, waymo_eval, waymo_eval2d  # noqa: E402
from cpd_amd.synthetic import waymo_infos  # noqa: E402

CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
MODULES = {"3d": waymo_eval, "2d": waymo_eval2d}


def threshold_sets(protocol, n):
    own = waymo_eval.BOX_TYPES[MODULES[protocol].OpenPCDetWaymoDetectionMetricsEstimator.BOX_TYPE][3]
    return [(round(own[0] - 0.1 * s, 1),) + tuple(own[1:]) for s in range(n)]


def evaluate(protocol, sets, pd_infos, gt_infos):
    """The protocol's waymo_evaluation, or waymo_evaluation_at when more than the protocol's own set is asked for."""
    est = MODULES[protocol].OpenPCDetWaymoDetectionMetricsEstimator()
    with contextlib.redirect_stdout(io.StringIO()):
        if len(sets) == 1:
            return est.waymo_evaluation(pd_infos, gt_infos, CLASSES, fake_gt_infos=False)
        return est.waymo_evaluation_at(pd_infos, gt_infos, CLASSES, sets, fake_gt_infos=False)[0]


def launch_ms(protocol, sets, pd_infos, gt_infos, reps):
    """Event times of the launches over the whole split as one chunk (the driver's own arrays, prepared once)."""
    est = MODULES[protocol].OpenPCDetWaymoDetectionMetricsEstimator()
    width, heading_col, iou_entry, _ = waymo_eval.BOX_TYPES[est.BOX_TYPE]
    n_frames = len(gt_infos)
    pf, pb, pt, ps, _, _ = est.generate_waymo_type_results(pd_infos, CLASSES, is_gt=False)
    gf, gb, gt, _, _, gd = est.generate_waymo_type_results(gt_infos, CLASSES, is_gt=True, fake_gt_infos=False)
    pd = waymo_eval._checked("prediction", pf, pb, pt, n_frames, width, score=(ps, np.float32))
    g = waymo_eval._checked("ground-truth", gf, gb, gt, n_frames, width, difficulty=(gd, np.uint8))
    pd, pd_n = waymo_eval._grouped(pd, n_frames)
    g, gt_n = waymo_eval._grouped(g, n_frames)
    dev, P, lib = waymo_eval._to_dev, _lib.ptr, _lib.lib()
    pair_off = waymo_eval._offsets(pd_n * gt_n, np.int64)
    n_q, n_pairs = len(pd_n), int(pair_off[-1])
    d_pb, d_gb = dev(pd["boxes"], np.float32), dev(g["boxes"], np.float32)
    d_po, d_go = dev(waymo_eval._offsets(pd_n, np.int32), np.int32), dev(waymo_eval._offsets(gt_n, np.int32), np.int32)
    d_pair = dev(pair_off, np.int64)
    d_ph, d_gh = dev(pd["boxes"][:, heading_col], np.float32), dev(g["boxes"][:, heading_col], np.float32)
    d_s, d_d = dev(pd["score"], np.float32), dev(g["difficulty"], np.uint8)
    iou = torch.empty(max(n_pairs, 1), dtype=torch.float64, device="cuda")
    counts = torch.zeros((len(sets), 4, 2, 101, 3), dtype=torch.int64, device="cuda")
    ha = torch.zeros((len(sets), 4, 2, 101), dtype=torch.float64, device="cuda")
    ws_bytes = lib.cpd_waymo_match_workspace_bytes(n_q, len(pd["score"]))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    thr = [(_lib._D * 4)(*one) for one in sets]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    iou_ms, match_ms = [], []
    for rep in range(reps + 1):                                  # the first pass warms up and is not reported
        ev[0].record()
        _lib.check(getattr(lib, iou_entry)(P(d_pb), P(d_gb), P(d_po), P(d_go), P(d_pair), n_q, n_pairs, P(iou), _lib.stream()),
                   iou_entry)
        ev[1].record()
        for s in range(len(sets)):
            _lib.check(lib.cpd_waymo_match(P(iou), P(d_pair), P(d_po), P(d_go), n_q, len(pd["score"]), len(g["difficulty"]),
                                           P(d_s), P(d_d), P(d_ph), P(d_gh), thr[s], int(pd_n.max()), int(gt_n.max()), 0,
                                           P(counts[s]), P(ha[s]), P(ws), ws_bytes, _lib.stream()), "cpd_waymo_match")
        ev[2].record()
        torch.cuda.synchronize()
        if rep:
            iou_ms.append(ev[0].elapsed_time(ev[1]))
            match_ms.append(ev[1].elapsed_time(ev[2]))
    return {"iou_ms": round(float(np.median(iou_ms)), 3), "iou_ms_min_max": [round(min(iou_ms), 3), round(max(iou_ms), 3)],
            "match_ms": round(float(np.median(match_ms)), 3), "match_ms_min_max": [round(min(match_ms), 3), round(max(match_ms), 3)],
            "event_reps": reps, "pairs": n_pairs, "problems": n_q, "max_pd": int(pd_n.max()), "max_gt": int(gt_n.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--protocol", choices=sorted(MODULES), default="3d")
    ap.add_argument("--threshold-sets", type=int, default=1)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--event-reps", type=int, default=9)
    ap.add_argument("--ref-frames", type=int, default=100)
    args = ap.parse_args()
    if args.threshold_sets < 1 or args.event_reps < 1:
        ap.error("--threshold-sets and --event-reps are at least 1")
    sets = threshold_sets(args.protocol, args.threshold_sets)
    torch.cuda.set_device(0)
    pd_infos, gt_infos = waymo_infos(args.frames, seed=1)
    result = evaluate(args.protocol, sets, pd_infos, gt_infos)   # warm-up (module load, allocator)
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate(args.protocol, sets, pd_infos, gt_infos)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    line = {"protocol": args.protocol, "threshold_sets": sets, "frames": args.frames,
            "pd": int(sum(len(i["name"]) for i in pd_infos)), "gt": int(sum(len(i["name"]) for i in gt_infos)),
            "end_to_end_s": round(float(np.median(times)), 4), "end_to_end_s_min_max": [round(min(times), 4), round(max(times), 4)]}
    line.update(launch_ms(args.protocol, sets, pd_infos, gt_infos, args.event_reps))
    line["vehicle_l2_ap"] = round(result["OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/AP"][0], 4)
    if args.ref_frames > 0 and len(sets) == 1:
        R = __import__("ref_waymo_eval" if args.protocol == "3d" else "ref_waymo_eval2d")
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})     # one core
        n = min(args.ref_frames, args.frames)
        t0 = time.perf_counter()
        ref = R.waymo_evaluation(pd_infos[:n], gt_infos[:n], CLASSES, fake_gt_infos=False)[0]
        line["ref_frames"], line["ref_one_core_s"] = n, round(time.perf_counter() - t0, 2)
        sub = evaluate(args.protocol, sets, pd_infos[:n], gt_infos[:n])
        line["ref_max_abs_diff"] = float(max(abs(sub[k][0] - ref[k][0]) for k in ref))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
