#!/usr/bin/env python3
"""Time the OYSTER generator's stages (cpd_amd.oyster) on a full-size synthetic sequence: cpd_amd.synthetic.ppscore_sequence at
Waymo azimuth resolution (64 x 2650 rays, float16 frames), OYSTER_GENERATOR_CONFIG (the yaml's).
  * stage_ms_per_frame: device time of ground, dbscan and boxes from HIP events around each stage of one chunk of `--chunk`
    frames (already on the device, file I/O excluded), after a warm-up pass; chain_ms_per_frame: OutlineGPU.frames_boxes by the
    host clock, upload and copy back included;
  * tracker_s: cpd_amd.tracker.TrackSmooth over every frame's raw boxes, then collect_tracks (every frame's
    get_current_frame_objects_and_cls and drop_cls), on the host;
  * align: the kept tracks of the sequence through cpd_oyster_align_tracks -- device time of the one launch from events (inputs
    on the device, after a warm-up launch), align_tracks by the host clock (upload and copy back included), and one core running
    the restatement (tests/ref_oyster.py, numpy, vectorised per track) on the same input, with the worst x, y difference and
    whether the other columns are the same bits;
  * align_full: the same three numbers for `--tracks` random tracks of `--track-len` boxes, the size of a whole Waymo segment
    (about 198 frames), which this short drive does not reach.
Prints one JSON line. Not part of bench.py. Usage: python tools/oyster_time.py [--frames 24] [--n-az 2650] [--chunk 12]"""
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

from cpd_amd import outline, oyster  # noqa: E402
from cpd_amd.synthetic import ppscore_sequence  # noqa: E402
from cpd_amd.tracker import TrackSmooth  # noqa: E402


def time_align(boxes, off):
    import ref_oyster as RO
    dev = torch.device("cuda")
    top = np.array([oyster.track_top(int(k)) for k in np.diff(off)], np.int32)
    d_box, d_off = torch.from_numpy(boxes).to(dev), torch.from_numpy(off.astype(np.int32)).to(dev)
    d_top, d_out = torch.from_numpy(top).to(dev), torch.empty_like(d_box)
    oyster.launch_align(d_box, d_off, d_top, d_out)                               # warm-up
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    oyster.launch_align(d_box, d_off, d_top, d_out)
    ev[1].record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = oyster.align_tracks(boxes, off)
    host = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = RO.align_tracks(boxes, off)
    rest = time.perf_counter() - t0
    return {"tracks": len(off) - 1, "boxes": len(boxes), "longest_track": int(np.diff(off).max()),
            "device_ms": round(ev[0].elapsed_time(ev[1]), 4), "host_call_ms": round(host * 1e3, 3),
            "restatement_ms": round(rest * 1e3, 3), "worst_xy_difference": float(np.abs(got[:, :2] - want[:, :2]).max()),
            "other_columns_same_bits": bool(np.array_equal(got[:, 2:].view(np.uint64), want[:, 2:].view(np.uint64)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--n-az", type=int, default=2650)
    ap.add_argument("--chunk", type=int, default=12)
    ap.add_argument("--tracks", type=int, default=150)
    ap.add_argument("--track-len", type=int, default=198)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "oyster_time.py needs a GPU"
    cfg = oyster.OYSTER_GENERATOR_CONFIG
    n, c = args.frames, min(args.chunk, args.frames)
    frames, poses = ppscore_sequence(41, n, args.n_az, np.float16, origin=(4200.0, -1800.0, 35.0))
    frames = [np.ascontiguousarray(f[:, 0:3]) for f in frames]
    g = outline.OutlineGPU(outline._params(cfg))
    g.frames_boxes(frames[:c])                                                    # warm-up: workspaces grow here
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    boxes = g.frames_boxes(frames[:c])
    chain = (time.perf_counter() - t0) / c
    for c0 in range(c, n, c):
        boxes += g.frames_boxes(frames[c0:c0 + c])

    pts, off, _ = g.upload(frames[:c])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    xyz, _, cnt, _ = g.ground(pts, off, c)
    ev[1].record()
    labels, ncl = g.dbscan(xyz, off, cnt, c)
    ev[2].record()
    g.boxes(xyz, off, cnt, labels, ncl, c, True, outline.BOX_CAP_PER_FRAME * c)
    ev[3].record()
    torch.cuda.synchronize()
    stage = {k: round(ev[i].elapsed_time(ev[i + 1]) / c, 3) for i, k in enumerate(["ground", "dbscan", "boxes"])}
    out = {"frames": n, "chunk": c, "points_per_frame": int(np.mean([len(f) for f in frames])),
           "non_ground_rows_per_frame": int(cnt.cpu().numpy().mean()),
           "raw_boxes_per_frame": round(float(np.mean([len(b) for b in boxes])), 1), "stage_ms_per_frame": stage,
           "stages_ms_per_frame": round(sum(stage.values()), 3), "chain_ms_per_frame": round(chain * 1e3, 3)}

    t0 = time.perf_counter()
    ts = TrackSmooth(cfg)
    ts.tracking([b.copy() if len(b) else [] for b in boxes], poses)
    tracks = oyster.collect_tracks(ts, n)
    out["tracker_s"] = round(time.perf_counter() - t0, 3)
    kept = [t for t in tracks.values() if len(t) >= oyster.MIN_TRACK_LEN]
    out["tracker_tracks"] = len(ts.tracker.active_trajectories) + len(ts.tracker.dead_trajectories)
    out["collected_tracks"], out["kept_tracks"] = len(tracks), len(kept)
    if kept:
        toff = np.zeros(len(kept) + 1, np.int64)
        toff[1:] = np.cumsum([len(t) for t in kept])
        out["align"] = time_align(np.array([e[0] for t in kept for e in t.values()]), toff)

    rng = np.random.default_rng(5)
    m = args.tracks * args.track_len
    ang, r = rng.uniform(-np.pi, np.pi, m), rng.uniform(2, 70, m)
    full = np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(-1, 3, m), rng.uniform(0.3, 12, m), rng.uniform(0.3, 3, m),
                     rng.uniform(0.5, 4, m), rng.uniform(-np.pi, np.pi, m)], 1)
    out["align_full"] = time_align(full, np.arange(args.tracks + 1, dtype=np.int64) * args.track_len)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
