#!/usr/bin/env python3
"""Time the two device stages of the KITTI transfer evaluation (cpd_amd.kitti2waymo, csrc/kitti2waymo.hip) against the same work in
numpy on the host: the FOV crop of 8 frames of 120 k points, and the export of 8 x 300 detections.
Prints one JSON line; every figure is the median of --reps runs after --warmup, on the same host in the same run:
  fov_host_ms           per frame Calibration.lidar_to_rect + get_fov_flag + the mask, the z shift and the zeroed features (numpy,
                        host clock): the work of Kitti2WaymoDataset.__getitem__'s point stage
  fov_call_ms           fov_points on host arrays: one packed upload, the launch pair, the read-back of the 8 counts; host clock
  fov_resident_ms       the same with the points already on the device; host clock
  fov_launch_event_ms   the launch pair alone on resident data, from HIP events
  export_host_ms        per frame the box edits, the centre shift (vectorised over the frame's boxes), boxes3d_lidar_to_kitti_camera,
                        boxes3d_kitti_camera_to_imageboxes and alpha in numpy; host clock
  export_call_ms        generate_prediction_dicts on device tensors: the launch, one copy back, the annos; host clock
  export_launch_event_ms  the launch alone on resident data, from HIP events
`fov_equal` / `export_equal`: the frames whose kept rows equal the host's bit for bit / whose kept names and scores equal the host's.
Not part of bench.py. Usage: python tools/kitti2waymo_time.py [--reps 5] [--warmup 1] [--frames 8] [--points 120000] [--boxes 300]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import kitti2waymo as K, ops  # noqa: E402

CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
CALIB = {"P2": np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32),
         "R0": np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]], np.float32),
         "Tr_velo2cam": np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                                  [0.9998621, 0.00752379, 0.01480755, -0.2717806]], np.float32)}
SHAPE = (375, 1242)


def host_fov(points, calib, shape):
    flag = K.get_fov_flag(calib.lidar_to_rect(points[:, 0:3]), shape, calib)
    out = points[flag] + [0, 0, K.SENSOR_LIFT, 0]
    out[:, 3:] = 0
    return out.astype(np.float32)


def host_export(boxes, scores, labels, calib, shape):
    """generate_single_sample_dict in numpy, the centre shift vectorised over the frame's label-1 boxes"""
    b = boxes.copy()
    b[:, 2] -= np.float32(1.55)
    b[:, 2] += np.float32(0.1)
    b[:, 3:5] -= np.float32(0.2)
    b[:, 5] -= np.float32(0.1)
    keep = b[:, 3] < 5
    b, scores, labels = b[keep], scores[keep], labels[keep]
    one = labels == 1
    half = (np.float32(0.1) + np.minimum(np.linalg.norm(b[:, :3], axis=1), np.float32(60)) / np.float32(60) * np.float32(0.3)) / np.float32(2)
    step = np.stack([half * np.cos(b[:, 6]), half * np.sin(b[:, 6])], 1).astype(np.float64)
    xy = b[:, :2].astype(np.float64)
    near = np.linalg.norm(xy + step, axis=1) < np.linalg.norm(xy - step, axis=1)
    b[one, :2] = np.where(near[:, None], xy + step, xy - step)[one]
    cam = K.boxes3d_lidar_to_kitti_camera(b, calib)
    img = K.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=shape)
    return {"name": np.array(CLASSES)[labels - 1], "score": scores, "alpha": -np.arctan2(-b[:, 1], b[:, 0]) + cam[:, 6], "bbox": img,
            "dimensions": cam[:, 3:6], "location": cam[:, 0:3], "rotation_y": cam[:, 6], "boxes_lidar": b}


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


def event_ms(fn, reps, warmup):
    ev = []
    for i in range(4 * reps + warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ev.append(e0.elapsed_time(e1))
    return round(float(np.median(ev)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--boxes", type=int, default=300)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(1)
    calibs, shapes = [K.Calibration(CALIB)] * args.frames, [SHAPE] * args.frames
    clouds = []
    for _ in range(args.frames):
        r, a = 70 * np.sqrt(rng.uniform(0.002, 1, args.points)), rng.uniform(-np.pi, np.pi, args.points)
        clouds.append(np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.5, 1.5, args.points), rng.uniform(0, 1, args.points)], 1).astype(np.float32))
    preds = []
    for _ in range(args.frames):
        n = args.boxes
        x = rng.uniform(6, 70, n)
        b = np.stack([x, x * rng.uniform(-0.6, 0.6, n), rng.uniform(0.3, 1.0, n), rng.uniform(0.6, 5.6, n), rng.uniform(0.6, 2.2, n),
                      rng.uniform(1.4, 1.9, n), rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
        preds.append({"pred_boxes": torch.from_numpy(b).cuda(), "pred_scores": torch.from_numpy(np.sort(rng.uniform(0.1, 1, n))[::-1].astype(np.float32)).cuda(),
                      "pred_labels": torch.from_numpy(rng.integers(1, 4, n)).cuda()})
    host_preds = [{k: v.cpu().numpy() for k, v in d.items()} for d in preds]
    batch = {"frame_id": ["%06d" % f for f in range(args.frames)], "calib": calibs, "image_shape": shapes}

    want = [host_fov(c, calibs[0], SHAPE) for c in clouds]
    got = K.fov_points(clouds, calibs, shapes)
    line = {"frames": args.frames, "points": args.points, "boxes": args.boxes, "reps": args.reps, "warmup": args.warmup,
            "kept_points": int(sum(len(g) for g in got)),
            "fov_equal": sum(int(np.array_equal(w.view(np.int32), g.cpu().numpy().view(np.int32))) for w, g in zip(want, got))}
    want = [host_export(d["pred_boxes"], d["pred_scores"], d["pred_labels"], calibs[0], SHAPE) for d in host_preds]
    got = K.generate_prediction_dicts(batch, preds, CLASSES)
    line["kept_boxes"] = int(sum(len(g["score"]) for g in got))
    line["export_equal"] = sum(int(np.array_equal(w["name"], g["name"]) and np.array_equal(w["score"], g["score"])) for w, g in zip(want, got))
    line["export_bbox_max_diff_px"] = round(float(max(np.abs(w["bbox"] - g["bbox"]).max() for w, g in zip(want, got) if len(w["score"]) == len(g["score"]))), 6)

    line["fov_host_ms"] = median_ms(lambda: [host_fov(c, calibs[0], SHAPE) for c in clouds], args.reps, args.warmup)
    line["fov_call_ms"] = median_ms(lambda: K.fov_points(clouds, calibs, shapes), args.reps, args.warmup)
    resident = [torch.from_numpy(c).cuda() for c in clouds]
    line["fov_resident_ms"] = median_ms(lambda: K.fov_points(resident, calibs, shapes), args.reps, args.warmup)
    packed = torch.cat(resident, 0)
    start_host = np.arange(args.frames + 1, dtype=np.int32) * args.points
    start, frames = K._upload_tables(start_host, K.frame_words(calibs, shapes), packed.device)
    out, count = ops.kitti_fov_points(packed, start, args.points, frames)
    ws = torch.empty((4096 + 4 * args.frames * (args.points // K.TILE + 1),), dtype=torch.uint8, device="cuda")
    line["fov_launch_event_ms"] = event_ms(lambda: ops.kitti_fov_points(packed, start, args.points, frames, out=out, out_count=count, workspace=ws),
                                           args.reps, args.warmup)
    line["export_host_ms"] = median_ms(lambda: [host_export(d["pred_boxes"], d["pred_scores"], d["pred_labels"], calibs[0], SHAPE) for d in host_preds],
                                       args.reps, args.warmup)
    line["export_call_ms"] = median_ms(lambda: K.generate_prediction_dicts(batch, preds, CLASSES), args.reps, args.warmup)
    boxes, scores, labels, seg_host = K._cat_predictions(preds)
    seg, frames = K._upload_tables(seg_host, K.frame_words(calibs, shapes), boxes.device)
    buf = ops.kitti_export(boxes, scores, labels, seg, frames)["buffer"]
    line["export_launch_event_ms"] = event_ms(lambda: ops.kitti_export(boxes, scores, labels, seg, frames, out=buf), args.reps, args.warmup)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
