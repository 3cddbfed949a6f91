#!/usr/bin/env python3
"""Time cpd_amd.outline (the DBSCAN pseudo-label generator) on float16 cpd_amd.synthetic.outline_scene frames (Waymo size):
  * per-stage device time (ground / DBSCAN / boxes) of one 16-frame call, from HIP events around each stage's launches;
  * frames/s of the batched path (outline_frames: launches, one read-back, host class chain) at 1 and 16 frames per call;
  * the single-process sequence driver (create_outline_boxes) end to end on a temporary 64-frame sequence, .npy reads included.
Prints one JSON line. Not part of bench.py. Usage: python tools/outline_time.py [--reps 5]"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import outline  # noqa: E402
from cpd_amd.synthetic import outline_scene  # noqa: E402

CFG = outline.DBSCAN_GENERATOR_CONFIG


def stage_ms(g, frames, reps):
    n = len(frames)
    pts, off, _ = g.upload(frames)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    acc = np.zeros(3)
    for r in range(reps + 1):
        ev[0].record()
        xyz, _, cnt, _ = g.ground(pts, off, n)
        ev[1].record()
        labels, ncl = g.dbscan(xyz, off, cnt, n)
        ev[2].record()
        g.boxes(xyz, off, cnt, labels, ncl, n, True, outline.BOX_CAP_PER_FRAME * n)
        ev[3].record()
        torch.cuda.synchronize()
        if r:
            acc += [ev[k].elapsed_time(ev[k + 1]) for k in range(3)]
    return dict(zip(("ground_ms", "dbscan_ms", "boxes_ms"), (acc / reps).round(3).tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    frames = [outline_scene(500 + k, np.float16) for k in range(16)]
    g = outline.OutlineGPU(outline._params(CFG))
    res = {"points_per_frame": int(np.mean([len(f) for f in frames])),
           "stages_16_frames": stage_ms(g, frames, args.reps)}
    for per_call in (1, 16):
        outline.outline_frames(frames[:per_call], CFG, gpu=g)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.reps):
            for c in range(0, 16, per_call):
                outline.outline_frames(frames[c:c + per_call], CFG, chunk=per_call, gpu=g)
        dt = (time.perf_counter() - t) / (args.reps * 16)
        res["frames_per_s_%d_per_call" % per_call] = round(1.0 / dt, 1)
        res["ms_per_frame_%d_per_call" % per_call] = round(dt * 1e3, 3)
    with tempfile.TemporaryDirectory() as root:
        seq = "segment-timing"
        os.makedirs(os.path.join(root, seq))
        for i in range(64):
            np.save(os.path.join(root, seq, "%04d.npy" % i), frames[i % 16])
        with open(os.path.join(root, seq, seq + ".pkl"), "wb") as f:
            pickle.dump([{} for _ in range(64)], f)
        cfg = dict(InitLabelGenerator="DBSCAN", GeneratorConfig=CFG)
        t = time.perf_counter()
        outline.create_outline_boxes([seq], root, cfg)
        dt = time.perf_counter() - t
        res["driver_64_frames_s"] = round(dt, 3)
        res["driver_ms_per_frame"] = round(dt / 64 * 1e3, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
