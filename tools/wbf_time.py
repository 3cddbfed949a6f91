#!/usr/bin/env python3
"""Time the fusion of test-time-augmentation views (cpd_amd.wbf, cpd_wbf_cluster) on a synthetic split: 6 views x 64 frames, about
50 objects per frame seen in 1..6 views (a few hundred boxes per frame), three classes with MERGE_TYPE (WBF-mean, WBF-max, WBF-mean).
Prints one JSON line; every figure is the median of --reps runs after --warmup, on the same host in the same run:
  a_host_loop_ms          the fusion as a numpy loop over the boxes, frame by frame and class by class (the work the reference's
                          merge_by_WBF / compute_WBF do: one 1 x K host IoU per box, one re-sum per join), on this library's host
                          boxes_bev_iou_cpu (cpd_boxes_iou_bev_cpu) and limit_period; host clock
  b_merge_frames_ms       merge_frames for the whole split: host segment table, one upload, one launch, one read-back, the per-frame
                          lists; host clock
  c_cluster_segments_ms   the upload, the launch and the read-back alone (cluster_segments on the prepared table); host clock
  d_launch_event_ms       the launch alone on resident data, from HIP events
`frames_equal` counts the frames whose fused result equals the loop's bit for bit (the loop's IoUs come from the host build of
the same expressions; a frame differs only where an IoU falls within rounding of a threshold).
Not part of bench.py. Usage: python tools/wbf_time.py [--reps 5] [--warmup 1] [--frames 64] [--views 6] [--objects 50]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import iou3d_nms_utils, ops, wbf  # noqa: E402
from cpd_amd.augmentor import limit_period  # noqa: E402

CLASSES = ("Car", "Pedestrian", "Cyclist")
SIZES = {"Car": (4.7, 2.1, 1.7), "Pedestrian": (0.9, 0.85, 1.75), "Cyclist": (1.8, 0.8, 1.7)}
CFG = {"WBF_IOUS": [0.55, 0.3, 0.4], "WBF_PRE_SCORES": [0.1, 0.1, 0.1], "MERGE_TYPE": ["WBF-mean", "WBF-max", "WBF-mean"], "NMS_IOU": 0.1}


def loop_compute_wbf(scores, boxes, iou_thresh, kind):
    """The fusion of one sorted segment as a host loop in this project's words (the shape of tests/ref_wbf.py's restatement): per
    box one 1 x K call of the host IoU against the clusters so far, per join of a 'mean' cluster a float64 re-sum over its members
    that starts from the box as merged so far. -> (scores, boxes) of the clusters in creation order."""
    f32 = np.float32
    boxes = boxes.copy()
    if len(scores):
        boxes[:, 6] = limit_period(boxes[:, 6], offset=0.5, period=2 * np.pi)
    merged, members = [], []
    for i in range(len(scores)):
        k, v = -1, f32(-1)
        if merged:
            v = iou3d_nms_utils.boxes_bev_iou_cpu(boxes[i:i + 1], np.array(merged, f32))[0]
            k = int(np.argmax(v))
            v = v[k]
        if v > f32(iou_thresh):
            members[k].append(i)
            if kind == "mean":
                acc, total = np.zeros(6, np.float64), f32(0)
                for pos, j in enumerate(members[k]):
                    acc += ((merged[k][:6] if pos == 0 else boxes[j, :6]) * scores[j]).astype(f32)
                    total = f32(total + scores[j])
                merged[k][:6] = (acc / np.float64(total)).astype(f32)
        else:
            merged.append(boxes[i].copy())
            members.append([i])
    out = []
    for m in members:
        if kind == "mean":
            total = f32(0)
            for j in m:
                total = f32(total + scores[j])
            out.append(f32(total / f32(len(m))))
        else:
            out.append(scores[m].max())
    return np.array(out, f32), np.array(merged, f32).reshape(-1, 7)


def loop_merge_frame(names, scores, boxes):
    """one frame: floor, sort and fuse every class of CFG, classes concatenated in order"""
    got = []
    for c, cls in enumerate(CLASSES):
        idx = wbf.segment_order(names, scores, cls, CFG["WBF_PRE_SCORES"][c])
        s, b = loop_compute_wbf(scores[idx], boxes[idx], CFG["WBF_IOUS"][c], "mean" if CFG["MERGE_TYPE"][c] == "WBF-mean" else "max")
        got.append((names[idx][:len(s)], s, b))
    return tuple(np.concatenate([g[k] for g in got]) for k in range(3))


def synthetic_views(seed, frames, views, objects):
    """-> list over views of per-frame annotation dicts: every object is detected in each view with probability 0.7, with a pose
    jitter of a few per cent of its size; every view adds a few false positives of its own"""
    rng = np.random.default_rng(seed)
    out = [[] for _ in range(views)]
    for f in range(frames):
        cls = rng.choice(len(CLASSES), objects, p=[0.6, 0.3, 0.1])
        base = np.zeros((objects, 7))
        base[:, :2] = rng.uniform(-70, 70, (objects, 2))
        base[:, 2] = rng.uniform(-1, 1, objects)
        base[:, 3:6] = np.array([SIZES[CLASSES[c]] for c in cls]) * np.exp(rng.normal(0, 0.1, (objects, 3)))
        base[:, 6] = rng.uniform(-np.pi, np.pi, objects)
        conf = rng.uniform(0.15, 0.95, objects)
        for v in range(views):
            seen = rng.uniform(size=objects) < 0.7
            b = base[seen].copy()
            n = len(b)
            b[:, :2] += rng.normal(0, 0.04, (n, 2)) * b[:, 3:5].min(1, keepdims=True)
            b[:, 3:6] *= np.exp(rng.normal(0, 0.03, (n, 3)))
            b[:, 6] += rng.normal(0, 0.03, n)
            s = np.clip(conf[seen] + rng.normal(0, 0.05, n), 0.02, 0.99)
            fp = int(rng.integers(2, 8))
            fb = np.zeros((fp, 7))
            fc = rng.choice(len(CLASSES), fp)
            fb[:, :2] = rng.uniform(-70, 70, (fp, 2))
            fb[:, 3:6] = np.array([SIZES[CLASSES[c]] for c in fc])
            fb[:, 6] = rng.uniform(-np.pi, np.pi, fp)
            out[v].append({"name": np.array([CLASSES[c] for c in np.concatenate([cls[seen], fc])]),
                           "score": np.concatenate([s, rng.uniform(0.05, 0.4, fp)]).astype(np.float32),
                           "boxes_lidar": np.concatenate([b, fb]).astype(np.float32), "frame_id": "%06d" % f})
    return out


def median_ms(fn, reps, warmup):
    out = []
    for i in range(reps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(out)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--objects", type=int, default=50)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    views = synthetic_views(1, args.frames, args.views, args.objects)
    frames = [tuple(np.concatenate([v[f][k] for v in views]) for k in ("name", "score", "boxes_lidar")) for f in range(args.frames)]

    def loop():
        return [loop_merge_frame(n, s, b) for n, s, b in frames]

    def fused():
        return wbf.merge_frames(views, CFG, CLASSES)

    want, got = loop(), fused()
    equal = sum(int(np.array_equal(w[0], g["name"]) and np.array_equal(w[1], g["score"]) and np.array_equal(w[2], g["boxes_lidar"]))
                for w, g in zip(want, got))
    table = wbf.build_segment_table([(n, s) for n, s, _ in frames], CFG, CLASSES)
    boxes = np.ascontiguousarray(np.concatenate([f[2] for f in frames])[table.order])
    scores = np.concatenate([f[1] for f in frames])[table.order]
    line = {"frames": args.frames, "views": args.views, "boxes_in": int(sum(len(f[1]) for f in frames)), "boxes_floored": int(len(scores)),
            "boxes_out": int(sum(len(g["score"]) for g in got)), "boxes_out_loop": int(sum(len(w[1]) for w in want)),
            "segments": int(len(table.start)), "largest_segment": int(table.count.max()), "frames_equal": equal, "reps": args.reps,
            "warmup": args.warmup}
    line["a_host_loop_ms"] = median_ms(loop, args.reps, args.warmup)
    line["b_merge_frames_ms"] = median_ms(fused, args.reps, args.warmup)
    line["c_cluster_segments_ms"] = median_ms(lambda: wbf.cluster_segments(boxes, scores, table.start, table.count, table.thresh, table.mode),
                                              args.reps, args.warmup)
    dev = [torch.from_numpy(a).cuda() for a in (boxes, scores, table.start, table.count, table.thresh, table.mode)]
    outs = ops.wbf_cluster(*dev)
    ws = torch.empty(ops.wbf_workspace_bytes(len(scores)), dtype=torch.uint8, device="cuda")
    ev = []
    for i in range(4 * args.reps + args.warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.wbf_cluster(*dev, out_boxes=outs[0], out_scores=outs[1], out_count=outs[2], cluster_of=outs[3], workspace=ws)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ev.append(e0.elapsed_time(e1))
    line["d_launch_event_ms"] = round(float(np.median(ev)), 4)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
