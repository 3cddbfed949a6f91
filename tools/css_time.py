#!/usr/bin/env python3
"""Time the C_PROTO refiner's first stage (cpd_amd.cproto, csrc/cproto.hip + the ground / DBSCAN kernels) on one frame's
boxes at full size: a float16 cpd_amd.synthetic.cproto_sequence sweep at Waymo azimuth resolution (64 x 2650 rays) with
the boxes of its 30 objects (the 10 'Dis_Small' ones are skipped, as the refiner skips them).
  * gpu_ms_per_frame: device time of one CProtoGPU.run (crop, density filter, window, ground removal, DBSCAN, cluster choice
    and cell counts for every box; the frame is already on the device, file I/O excluded), from HIP events around `reps`
    back-to-back calls after a warm-up -- the one size read-back and the copy of the results lie inside the interval;
  * wall_ms_per_frame: the same calls by the host clock;
  * where scipy imports: restatement_s_per_frame, one core running tests/ref_cproto.py (cKDTree density filter, numpy ground
    removal and DBSCAN) over the same boxes on the same machine, whether its stages equal the GPU's, and the ratio.
Prints one JSON line. Not part of bench.py. Usage: python tools/css_time.py [--reps 10] [--n-az 2650]"""
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

from cpd_amd import cproto  # noqa: E402
from cpd_amd.synthetic import cproto_sequence  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-az", type=int, default=2650)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "css_time.py needs a GPU"
    cfg = cproto.CPROTO_CONFIG
    frames, infos = cproto_sequence(31, n_az=args.n_az, dtypes=(np.float16,))
    predefined = cfg["RefinerConfig"]["CSSConfig"]["PredifinedSize"]
    xyz = np.ascontiguousarray(frames[0][:, 0:3])
    boxes, names = [], []
    for box, name in zip(infos[0]["outline_box"], infos[0]["outline_cls"]):
        if name not in cproto.CLASSES:
            continue
        box = box.copy()
        if name == 'Pedestrian':
            box[3:5] = predefined['Pedestrian'][0:2]
        if name == 'Cyclist':
            box[4] = predefined['Cyclist'][1]
        boxes.append(box)
        names.append(name)
    boxes = np.array(boxes)
    seg_frame = np.zeros(len(boxes), np.int32)
    g = cproto.CProtoGPU(cfg)
    up = g.upload([xyz])
    for _ in range(2):
        res = g.run(up, boxes, seg_frame, stages=True)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.reps):
        g.run(up, boxes, seg_frame)
    ev1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.reps
    out = {"points": len(xyz), "boxes": len(boxes), "crop_rows": int(sum(len(c) for c in res["crop_src"])),
           "largest_crop": int(max(len(c) for c in res["crop_src"])), "scored": int((res["best_label"] >= 0).sum()),
           "reps": args.reps, "gpu_ms_per_frame": round(ev0.elapsed_time(ev1) / args.reps, 3),
           "wall_ms_per_frame": round(wall * 1e3, 3)}
    try:
        if args.no_restatement:
            raise ImportError("skipped")
        import scipy
        import ref_cproto as R
        t0 = time.perf_counter()
        segs = [R.segment(xyz, b, cfg) for b in boxes]
        sec = time.perf_counter() - t0
        same = all(np.array_equal(s[k], res[k][i]) for i, s in enumerate(segs)
                   for k in ("crop_src", "dens_mask", "filt_src", "ng_src", "labels", "cluster_src", "occ", "new_box"))
        out.update({"scipy": scipy.__version__, "restatement_s_per_frame": round(sec, 3), "stages_equal_restatement": bool(same),
                    "ratio": round(sec * 1e3 / out["gpu_ms_per_frame"], 1)})
    except ImportError as e:
        out["restatement"] = "not run (%s)" % e
    print(json.dumps(out))


if __name__ == "__main__":
    main()
