#!/usr/bin/env python3
"""Time test-time augmentation around an engine step at full size: the six shipped TEST_AUGMENTOR views (rotation 0 / +-0.3927, each
with and without the x flip) of --frames Waymo-sized frames, i.e. one engine step on 6 x frames frames, with the CenterPoint engine and
with the two-stage VoxelRCNN engine. Prints one JSON line per engine; every figure is the median of --reps runs after --warmup, host
clock around a device synchronisation, on the same host in the same run:
  engine_ms          the engine step alone on the view-major batch (views made beforehand)
  tta_engine_ms      cpd_amd.tta.TTAEngine.forward: cpd_tta_views, the engine step, cpd_tta_collect, cpd_wbf_cluster / cpd_nms_batch, one
                     read-back of the segment counts, the per-frame device slices
  composition_ms     the same by hand: TestAugmentor.forward per view and frame (one cpd_augment_scene launch and one blocking read of its
                     count each), the engine step on the same batch, per (view, frame) the read-back of the results and
                     TestAugmentor.backward in numpy, wbf.merge_frames (host segment table, one upload, one launch, one read-back)
  *_outside_engine   the share of the step that is not the engine step
`--composition-only` leaves cpd_amd.tta alone, so that the script also runs on a commit that does not have it yet.
Not part of bench.py. Usage: python tools/tta_time.py [--reps 5] [--warmup 2] [--frames 8] [--points 160000] [--composition-only]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import models, wbf  # noqa: E402
from cpd_amd.augmentor import TestAugmentor  # noqa: E402
from cpd_amd.engine import CenterPointEngine, ModelConfig, init_state_dict  # noqa: E402
from cpd_amd.synthetic import waymo_cloud  # noqa: E402
from cpd_amd.two_stage import VoxelRCNNEngine  # noqa: E402

CLASSES = ("Vehicle", "Pedestrian", "Cyclist")
ROT = 0.39269908169872414
VIEWS = [[dict(NAME="world_rotation", WORLD_ROT=rot), dict(NAME="world_flip", ALONG_AXIS=axis), dict(NAME="world_scaling", WORLD_SCALE=1)]
         for axis in ("None", "x") for rot in (0, ROT, -ROT)]
MERGE = {"WBF_IOUS": [0.55, 0.3, 0.4], "WBF_PRE_SCORES": [0.1, 0.1, 0.1], "MERGE_TYPE": ["WBF-mean", "WBF-max", "WBF-mean"], "NMS_IOU": 0.1}


def engines(dev):
    cfg = ModelConfig()
    sd = init_state_dict(cfg, 0)
    yield "centerpoint", CenterPointEngine(cfg, sd, device=dev)
    mcfg = models.waymo_voxel_rcnn_cfg()
    torch.manual_seed(0)
    head = models.__all__[mcfg.ROI_HEAD.NAME](input_channels={"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 128}, model_cfg=mcfg.ROI_HEAD,
                                              point_cloud_range=cfg.point_cloud_range, voxel_size=cfg.voxel_size, num_class=1)
    sd2 = dict(sd, **{"roi_head." + k: v.detach().clone() for k, v in head.state_dict().items()})
    yield "voxel_rcnn", VoxelRCNNEngine(cfg, mcfg.ROI_HEAD, mcfg.POST_PROCESSING, sd2, device=dev)


def median_ms(fn, reps, warmup):
    out = []
    for i in range(reps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(out)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=160000)
    ap.add_argument("--composition-only", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    clouds = [torch.from_numpy(waymo_cloud(200 + i, n_points=args.points)).to(dev) for i in range(args.frames)]
    augs = [TestAugmentor(v, CLASSES) for v in VIEWS]
    names = np.array(("",) + CLASSES)              # a label outside the class list (0: a padded RoI slot that survived) names no class
    b = len(clouds)
    for name, engine in engines(dev):
        def make_views():
            return [a.forward(dict(points=p))["points"] for a in augs for p in clouds]

        def composition():
            res = engine.forward(make_views())
            infos = [[dict(name=names[res[v * b + f]["pred_labels"].cpu().numpy().clip(0, len(CLASSES))], score=res[v * b + f]["pred_scores"].cpu().numpy(),
                           boxes_lidar=a.backward(dict(boxes_lidar=res[v * b + f]["pred_boxes"].cpu().numpy().copy()))["boxes_lidar"])
                      for f in range(b)] for v, a in enumerate(augs)]
            return wbf.merge_frames(infos, MERGE, CLASSES)

        batch = make_views()
        line = {"engine": name, "frames": b, "views": len(augs), "points": args.points, "reps": args.reps, "warmup": args.warmup}
        line["engine_ms"] = median_ms(lambda: engine.forward(batch), args.reps, args.warmup)
        line["composition_ms"] = median_ms(composition, args.reps, args.warmup)
        line["composition_outside_engine"] = round(1 - line["engine_ms"] / line["composition_ms"], 3)
        line["boxes_out_composition"] = int(sum(len(f["score"]) for f in composition()))
        if not args.composition_only:
            from cpd_amd import tta
            fused = tta.TTAEngine(engine, VIEWS, MERGE, CLASSES, max_batch=len(augs) * b)
            line["tta_engine_ms"] = median_ms(lambda: fused.forward(clouds), args.reps, args.warmup)
            line["tta_engine_outside_engine"] = round(1 - line["engine_ms"] / line["tta_engine_ms"], 3)
            line["boxes_out_tta_engine"] = int(sum(len(r["pred_scores"]) for r in fused.forward(clouds)))
        print(json.dumps(line), flush=True)
        del engine
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
