#!/usr/bin/env python3
"""Time refine_box_size's per-box work (cpd_amd.cproto_refine.RefineGPU.run: the first stage's kernels with the prototype size
fit and the orientation / drift kernels of csrc/cproto_refine.hip) on one frame's boxes at full size: a float16
cpd_amd.synthetic.cproto_sequence sweep at Waymo azimuth resolution (64 x 2650 rays) with the boxes of its 30 objects as the
first stage leaves them (the 10 'Dis_Small' ones are skipped, as the refiner skips them) and the prototypes the first stage and
construct_prototypes make of that frame.
  * gpu_ms_per_frame: device time of one RefineGPU.run (the frame is already on the device, file I/O excluded), from HIP events
    around `reps` back-to-back calls after a warm-up -- the one size read-back and the copy of the results lie inside the interval;
  * wall_ms_per_frame: the same calls by the host clock;
  * where scipy imports: restatement_s_per_frame, one core running tests/ref_cproto_refine.py (on top of tests/ref_cproto.py:
    cKDTree density filter, numpy ground removal and DBSCAN, then the fit, the cell counts, correct_orientation and
    density_guided_drift twice) over the same boxes on the same machine, whether its results equal the GPU's (fit_index, the
    chosen cluster and the fitted box exactly, the three refined boxes within 1e-9), and the ratio.
Prints one JSON line. Not part of bench.py. Usage: python tools/cproto_refine_time.py [--reps 10] [--n-az 2650]"""
import argparse
import copy
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import cproto, cproto_refine  # noqa: E402
from cpd_amd.synthetic import cproto_sequence  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-az", type=int, default=2650)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cproto_refine_time.py needs a GPU"
    cfg = copy.deepcopy(cproto_refine.REFINE_CONFIG)
    # the synthetic boxes score 0.4 .. 0.9: thresholds inside that range, so that every kind of fit and both boxes occur
    cfg["RefinerConfig"]["BasicProtoScoreThresh"] = {'Vehicle': 0.6, 'Pedestrian': 0.6, 'Cyclist': 2.0}
    cfg["RefinerConfig"]["OrienThresh"] = 0.6
    rcfg = cfg["RefinerConfig"]
    seq = "segment-00000031_time"
    frames, infos = cproto_sequence(31, n_az=args.n_az, dtypes=(np.float16,))
    xyz = np.ascontiguousarray(frames[0][:, 0:3])
    driver = cproto_refine.C_PROTO(seq, "/nonexistent", cfg)
    raw = {c: {} for c in cproto.CLASSES}
    driver.score_frames([xyz], infos, raw)                        # the first stage: _CSS infos and raw prototypes
    proto = cproto.construct_prototypes(raw, rcfg)
    table = cproto_refine.PrototypeTable(proto, rcfg["CSSConfig"]["PredifinedSize"])
    boxes, names, seg_cls, basic, pids = [], [], [], [], []
    for box, name, ob_id in zip(infos[0]["outline_box"], infos[0]["outline_cls"], infos[0]["outline_ids"]):
        if name not in cproto.CLASSES:
            continue
        pid = int(str(int(seq[8:16])) + str(ob_id))
        boxes.append(np.array(box)), names.append(name), seg_cls.append(cproto.CLASSES.index(name))
        basic.append(table.basic_whl(name, pid)), pids.append(pid)
    boxes, basic = np.array(boxes), np.array(basic)
    seg_frame = np.zeros(len(boxes), np.int32)
    g = driver.gpu
    g.set_prototypes(table)
    up = g.upload([xyz])
    for _ in range(2):
        res = g.run(up, boxes, seg_frame, seg_cls=seg_cls, basic_whl=basic)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.reps):
        g.run(up, boxes, seg_frame, seg_cls=seg_cls, basic_whl=basic)
    ev1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.reps
    fit = res["fit_index"]
    out = {"points": len(xyz), "boxes": len(boxes), "with_cluster": int((res["best_label"] >= 0).sum()),
           "cluster_rows": int(res["best_count"].sum()), "largest_cluster": int(res["best_count"].max()),
           "fit_own": int((fit == -2).sum()), "fit_high_quality": int((fit >= 0).sum()), "fit_predefined": int((fit == -1).sum()),
           "reps": args.reps, "gpu_ms_per_frame": round(ev0.elapsed_time(ev1) / args.reps, 3),
           "wall_ms_per_frame": round(wall * 1e3, 3)}
    try:
        if args.no_restatement:
            raise ImportError("skipped")
        import scipy
        import ref_cproto_refine as RR
        tables = RR.hq_tables(proto)
        t0 = time.perf_counter()
        segs = [RR.refine_segment(xyz, b, n, p, tables, cfg) for b, n, p in zip(boxes, names, pids)]
        sec = time.perf_counter() - t0
        same, worst = True, 0.0
        for i, s in enumerate(segs):
            same &= s["fit_index"] == fit[i] and (s["best_label"] >= 0) == (res["best_label"][i] >= 0)
            same &= np.array_equal(s["fitted"], res["new_box"][i])
            if s["score"] is not None:
                same &= np.array_equal(s["occ"], res["occ"][i])
            if "box_drift" in s:
                worst = max(worst, max(float(np.abs(s[k] - res[k][i]).max()) for k in ("box_drift", "box_orient", "box_orient_drift")))
        out.update({"scipy": scipy.__version__, "restatement_s_per_frame": round(sec, 3),
                    "results_equal_restatement": bool(same and worst <= 1e-9), "worst_box_difference": worst,
                    "ratio": round(sec * 1e3 / out["gpu_ms_per_frame"], 1)})
    except ImportError as e:
        out["restatement"] = "not run (%s)" % e
    print(json.dumps(out))


if __name__ == "__main__":
    main()
