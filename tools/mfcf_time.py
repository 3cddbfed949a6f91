#!/usr/bin/env python3
"""Time the MFCF generator's stages (cpd_amd.mfcf) on a full-size synthetic sequence: cpd_amd.synthetic.ppscore_sequence at Waymo
azimuth resolution (64 x 2650 rays, float16 frames), PP scores from cpd_amd.ppscore (max_win 5, win_inte 1 on this short drive),
MFCF_GENERATOR_CONFIG (window of 10 sweeps, threshold 0.7).
  * stage_ms_per_frame: device time of gather, voxel_sample, ground, dbscan, boxes and fit_dgd from HIP events around each
    stage of one chunk holding every frame (the sweeps are already on the device, file I/O excluded), after a warm-up pass;
    chain_ms_per_frame: MFCFGPU.frames_boxes by the host clock, the copy back included;
  * rows: aggregated, voxel-sampled and non-ground rows per frame, boxes per frame;
  * tracker_s: cpd_amd.tracker.TrackSmooth over the sequence's per-frame boxes plus every frame's
    get_current_frame_objects_and_cls, on the host;
  * restatement_s_per_frame: one core running tests/ref_mfcf.py (numpy; the reference's own voxel_sampling is a Python loop
    over every row and would be slower still) over `--restate` frames of the same sequence on the same machine, whether its
    voxel-sampled rows equal the GPU's bit for bit and its boxes within 1e-9, and the ratio.
Prints one JSON line. Not part of bench.py. Usage: python tools/mfcf_time.py [--frames 12] [--n-az 2650] [--restate 1]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import mfcf, outline, ppscore  # noqa: E402
from cpd_amd.synthetic import ppscore_sequence  # noqa: E402
from cpd_amd.tracker import TrackSmooth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--n-az", type=int, default=2650)
    ap.add_argument("--restate", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mfcf_time.py needs a GPU"
    cfg = mfcf.MFCF_GENERATOR_CONFIG
    n = args.frames
    frames, poses = ppscore_sequence(41, n, args.n_az, np.float16, origin=(4200.0, -1800.0, 35.0))
    pp = ppscore.PPScoreGPU()
    dev_frames = [pp.upload(f) for f in frames]
    scores = []
    for i in range(n):
        js = [j for j in range(i - 5, i + 5) if 0 <= j < n]
        _, h = pp.run(dev_frames[i], [dev_frames[j] for j in js], [poses[j] for j in js], np.linalg.inv(poses[i]), 0.3,
                      want_counts=False)
        scores.append(h.cpu().numpy())
    del dev_frames, pp
    g = mfcf.MFCFGPU(cfg)
    sweeps = [g.upload(f, h) for f, h in zip(frames, scores)]
    wins = [mfcf.window(i, cfg["frame_num"], cfg["frame_interval"], lambda j: j < n) for i in range(n)]
    cur = list(range(n))
    boxes = g.frames_boxes(sweeps, poses, wins, cur, cfg["ppscore_thresh"])       # warm-up: workspaces grow here
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    boxes, bits, vox = g.frames_boxes(sweeps, poses, wins, cur, cfg["ppscore_thresh"], stages=True)
    chain = (time.perf_counter() - t0) / n

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    F1, cap = n + 1, outline.BOX_CAP_PER_FRAME * n
    ev[0].record()
    rows, off, count, _ = g.gather(sweeps, poses, wins, cur, cfg["ppscore_thresh"])
    ev[1].record()
    v, _, v_off, _ = g.voxel_sample(rows, off, count, n)
    ev[2].record()
    xyz, _, cnt, _ = g.ol.ground(v, v_off, F1)
    ev[3].record()
    labels, ncl = g.ol.dbscan(xyz, v_off, cnt, F1)
    ev[4].record()
    bx = g.ol.boxes(xyz, v_off, cnt, labels, ncl, F1, True, cap)
    ev[5].record()
    g.fit_dgd(xyz, v_off, cnt, labels, bx, F1, cap)
    ev[6].record()
    torch.cuda.synchronize()
    names = ["gather", "voxel_sample", "ground", "dbscan", "boxes", "fit_dgd"]
    stage = {k: round(ev[i].elapsed_time(ev[i + 1]) / n, 3) for i, k in enumerate(names)}
    out = {"frames": n, "points_per_frame": int(np.mean([len(f) for f in frames])),
           "aggregated_rows_per_frame": int(count.cpu().numpy().mean()), "voxel_rows_per_frame": int(np.mean([len(x) for x in vox])),
           "non_ground_rows_per_frame": int(cnt.cpu().numpy()[:n].mean()), "boxes_per_frame": round(float(np.mean([len(b) for b in boxes])), 1),
           "stage_ms_per_frame": stage, "stages_ms_per_frame": round(sum(stage.values()), 3),
           "dominant_stage": max(stage, key=stage.get), "chain_ms_per_frame": round(chain * 1e3, 3)}
    t0 = time.perf_counter()
    ts = TrackSmooth(cfg)
    ts.tracking([b.copy() if len(b) else [] for b in boxes], poses)
    final = [ts.get_current_frame_objects_and_cls(i) for i in range(n)]
    out["tracker_s"] = round(time.perf_counter() - t0, 3)
    out["tracks"] = len(ts.tracker.active_trajectories) + len(ts.tracker.dead_trajectories)
    out["final_boxes_per_frame"] = round(float(np.mean([len(f[0]) for f in final])), 1)
    if args.restate > 0:
        import ref_mfcf as RM
        pick = list(range(n))[n // 2:n // 2 + args.restate]
        same_vox, worst, same_count = True, 0.0, True
        t0 = time.perf_counter()
        for i in pick:
            agg = RM.gather(frames, scores, poses, i, RM.window(i, cfg["frame_num"], cfg["frame_interval"], n), cfg["ppscore_thresh"])
            rb, _, rv = RM.frame_boxes(agg, cfg, stages=True)
            same_vox &= rv.shape == vox[i].shape and np.array_equal(rv.view(np.uint32), vox[i].view(np.uint32))
            if len(rb) == len(boxes[i]):
                worst = max(worst, float(np.abs(np.asarray(rb).reshape(-1, 7) - np.asarray(boxes[i]).reshape(-1, 7)).max()) if len(rb) else 0.0)
            else:
                same_count = False
        sec = (time.perf_counter() - t0) / len(pick)
        out.update({"restated_frames": pick, "restatement_s_per_frame": round(sec, 2), "voxel_rows_equal": bool(same_vox),
                    "box_counts_equal": bool(same_count), "worst_box_difference": worst,
                    "ratio": round(sec * 1e3 / (chain * 1e3), 1)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
