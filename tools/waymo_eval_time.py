#!/usr/bin/env python3
"""Time cpd_amd.waymo_eval on a synthetic Waymo-format split (cpd_amd.synthetic.waymo_infos: 2000 frames, about 150
predictions and 60 ground truths per frame, mixed types). Prints one JSON line: the whole waymo_evaluation by the host
clock (median of --reps calls after one warm-up), both launches (cpd_waymo_iou, cpd_waymo_match) from HIP events over
the prepared arrays of the whole split, and the numpy / scipy restatement (tests/ref_waymo_eval.py) on one core of the
same host on a --ref-frames subset. There is no official-tool or parent-commit number to compare with.
Not part of bench.py. Usage: python tools/waymo_eval_time.py [--frames 2000] [--reps 3] [--ref-frames 100]"""
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

from cpd_amd import _lib, waymo_eval  # noqa: E402
from cpd_amd.synthetic import waymo_infos  # noqa: E402

CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]


def evaluate(pd_infos, gt_infos):
    est = waymo_eval.OpenPCDetWaymoDetectionMetricsEstimator()
    with contextlib.redirect_stdout(io.StringIO()):
        return est.waymo_evaluation(pd_infos, gt_infos, CLASSES, fake_gt_infos=False)


def launch_ms(pd_infos, gt_infos):
    """Event times of the two launches over the whole split as one chunk (the driver's own arrays, prepared once)."""
    est = waymo_eval.OpenPCDetWaymoDetectionMetricsEstimator()
    n_frames = len(gt_infos)
    pf, pb, pt, ps, _, _ = est.generate_waymo_type_results(pd_infos, CLASSES, is_gt=False)
    gf, gb, gt, _, _, gd = est.generate_waymo_type_results(gt_infos, CLASSES, is_gt=True, fake_gt_infos=False)
    pd = waymo_eval._checked("prediction", pf, pb, pt, n_frames, score=(ps, np.float32))
    g = waymo_eval._checked("ground-truth", gf, gb, gt, n_frames, difficulty=(gd, np.uint8))
    pd, pd_n = waymo_eval._grouped(pd, n_frames)
    g, gt_n = waymo_eval._grouped(g, n_frames)
    dev, P, lib = waymo_eval._to_dev, _lib.ptr, _lib.lib()
    pair_off = waymo_eval._offsets(pd_n * gt_n, np.int64)
    n_q, n_pairs = len(pd_n), int(pair_off[-1])
    d_pb, d_gb = dev(pd["boxes"], np.float32), dev(g["boxes"], np.float32)
    d_po, d_go = dev(waymo_eval._offsets(pd_n, np.int32), np.int32), dev(waymo_eval._offsets(gt_n, np.int32), np.int32)
    d_pair = dev(pair_off, np.int64)
    d_ph, d_gh = dev(pd["boxes"][:, 6], np.float32), dev(g["boxes"][:, 6], np.float32)
    d_s, d_d = dev(pd["score"], np.float32), dev(g["difficulty"], np.uint8)
    iou = torch.empty(max(n_pairs, 1), dtype=torch.float64, device="cuda")
    counts = torch.zeros((4, 2, 101, 3), dtype=torch.int64, device="cuda")
    ha = torch.zeros((4, 2, 101), dtype=torch.float64, device="cuda")
    ws_bytes = lib.cpd_waymo_match_workspace_bytes(n_q, len(pd["score"]))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    thr = (_lib._D * 4)(*waymo_eval.IOU_THRESHOLDS)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    out = {}
    for rep in range(2):                                         # the second pass is the one reported
        ev[0].record()
        _lib.check(lib.cpd_waymo_iou(P(d_pb), P(d_gb), P(d_po), P(d_go), P(d_pair), n_q, n_pairs, P(iou), _lib.stream()),
                   "cpd_waymo_iou")
        ev[1].record()
        _lib.check(lib.cpd_waymo_match(P(iou), P(d_pair), P(d_po), P(d_go), n_q, len(pd["score"]), len(g["difficulty"]), P(d_s),
                                       P(d_d), P(d_ph), P(d_gh), thr, int(pd_n.max()), int(gt_n.max()), 0, P(counts), P(ha),
                                       P(ws), ws_bytes, _lib.stream()), "cpd_waymo_match")
        ev[2].record()
        torch.cuda.synchronize()
        out = {"iou_ms": round(ev[0].elapsed_time(ev[1]), 3), "match_ms": round(ev[1].elapsed_time(ev[2]), 3)}
    out.update(pairs=n_pairs, problems=n_q, max_pd=int(pd_n.max()), max_gt=int(gt_n.max()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-frames", type=int, default=100)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    pd_infos, gt_infos = waymo_infos(args.frames, seed=1)
    result = evaluate(pd_infos, gt_infos)                        # warm-up (module load, allocator)
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate(pd_infos, gt_infos)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    line = {"frames": args.frames, "pd": int(sum(len(i["name"]) for i in pd_infos)),
            "gt": int(sum(len(i["name"]) for i in gt_infos)), "end_to_end_s": round(float(np.median(times)), 4)}
    line.update(launch_ms(pd_infos, gt_infos))
    line["vehicle_l2_ap"] = round(result["OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/AP"][0], 4)
    if args.ref_frames > 0:
        import ref_waymo_eval as R
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})     # one core
        n = min(args.ref_frames, args.frames)
        t0 = time.perf_counter()
        ref, _, _ = R.waymo_evaluation(pd_infos[:n], gt_infos[:n], CLASSES, fake_gt_infos=False)
        line["ref_frames"], line["ref_one_core_s"] = n, round(time.perf_counter() - t0, 2)
        sub = evaluate(pd_infos[:n], gt_infos[:n])
        line["ref_max_abs_diff"] = float(max(abs(sub[k][0] - ref[k][0]) for k in ref))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
