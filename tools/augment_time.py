#!/usr/bin/env python3
"""Time the training-time augmentor (cpd_amd.augmentor) on a full-size synthetic frame: three cpd_amd.synthetic.waymo_cloud
sweeps merged (about 480 k points, 5 columns), the OYSTER yaml's augmentor list (gt_sampling with SAMPLE_GROUPS 30 + 20 + 20,
flip, rotation, scaling) over a synthetic object database whose boxes sit on a grid (so every sample is accepted), then the
range mask and the shuffle.
  * prepare_ms: prepare_train_points per frame by the host clock with a device synchronise at the end, points already on the
    device -- database not resident (the sampled .bin files are read and uploaded per frame, as the reference reads them) and
    resident; median of `--repeats` frames after `--warmup` frames;
  * kernel_ms: device time of the one cpd_augment_scene call of such a frame, from HIP events;
  * restatement_ms: the same frames through the numpy restatement (tests/ref_augment.py under host_kernels) on one core of this
    host, median of `--host-repeats`;
  * database: create_track_groundtruth_database per frame (one 160 k sweep, `--db-boxes` boxes per class), device path against
    the restatement's transcription of the reference loop.
Prints one JSON line. Not part of bench.py. Usage: python tools/augment_time.py [--repeats 20] [--host-repeats 3]"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_augment as RA  # noqa: E402
from cpd_amd import augmentor as A  # noqa: E402
from cpd_amd.synthetic import waymo_cloud  # noqa: E402

PCR = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
SIZES = {"Vehicle": (4.6, 2.0, 1.7, 400), "Pedestrian": (0.7, 0.7, 1.75, 80), "Cyclist": (1.8, 0.8, 1.7, 150)}


def write_database(root, per_class=100, seed=3):
    """Objects on an 8 m grid (no two boxes overlap), `per_class` per class, points uniform inside the box."""
    rng = np.random.default_rng(seed)
    grid = [(x, y) for x in np.arange(-68, 69, 8.0) for y in np.arange(-68, 69, 8.0) if abs(x) > 6 or abs(y) > 6]
    order = rng.permutation(len(grid))
    db, at, rows = {c: [] for c in RA.CLASSES}, 0, 0
    for c in RA.CLASSES:
        l, w, h, npts = SIZES[c]
        for j in range(per_class):
            x, y = grid[order[at % len(grid)]]
            at += 1
            box = np.array([x, y, h / 2, l, w, h, rng.uniform(-np.pi, np.pi)])
            n = int(npts * rng.uniform(0.5, 1.5))
            pts = np.zeros((n, 5), np.float32)
            pts[:, :3] = rng.uniform(-0.5, 0.5, (n, 3)) * np.array([l, w, h])
            pts[:, 3:] = rng.uniform(0, 1, (n, 2))
            rel = os.path.join("pcdet_gt_track_database_train_cp", "seg", str(j), "%s_%d.bin" % (c, j))
            os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
            pts.tofile(os.path.join(root, rel))
            rows += n
            db[c].append({"name": c, "path": rel, "box3d_lidar": box, "num_points_in_gt": n, "difficulty": 1,
                          "labeling_method_dict": ["unlabeled"]})
    with open(os.path.join(root, "pcdet_waymo_track_dbinfos_train_cp.pkl"), "wb") as f:
        pickle.dump(db, f)
    return rows


def config():
    cfg = RA.augmentor_config()
    cfg["AUG_CONFIG_LIST"][0] = RA.sampler_config(("Vehicle:30", "Pedestrian:20", "Cyclist:20"))
    return cfg


def time_prepare(mod, root, frames, device, resident, warmup, repeats, sync):
    aug = mod.DataAugmentor(root, config(), RA.CLASSES, dataset_cfg=dict(current_label_method="unlabeled"), device=device,
                            resident=resident)
    np.random.seed(0)
    times, pasted, kept = [], [], []
    for it in range(warmup + repeats):
        pts = frames[it % len(frames)]
        d = dict(points=pts, gt_boxes=np.zeros((0, 7), np.float32), gt_names=np.zeros((0,), dtype=str))
        sync()
        t0 = time.perf_counter()
        d = mod.prepare_train_points(d, PCR, True, augmentor=aug)
        sync()
        if it >= warmup:
            times.append(time.perf_counter() - t0)
            pasted.append(len(aug.data_augmentor_queue[0].last_sampled))
            kept.append(int(d["points"].shape[0]))
    return round(float(np.median(times)) * 1e3, 3), float(np.mean(pasted)), int(np.mean(kept))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--db-boxes", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "augment_time.py needs a GPU"
    dev = torch.device("cuda")
    torch.set_num_threads(1)
    host_frames = [np.concatenate([waymo_cloud(3 * f + s, 160000) for s in range(3)]) for f in range(3)]
    dev_frames = [torch.from_numpy(f).to(dev) for f in host_frames]
    out = {"points_per_frame": int(host_frames[0].shape[0]), "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        out["database_points"] = write_database(root)
        for res in (False, True):
            ms, pasted, kept = time_prepare(A, root, dev_frames, dev, res, args.warmup, args.repeats, torch.cuda.synchronize)
            out["prepare_ms_resident" if res else "prepare_ms"] = ms
            out["pasted_objects"], out["rows_kept"] = pasted, kept
        # device time of the kernel call alone: one frame's paste through the sampler, then events around PointOps.run
        aug = A.DataAugmentor(root, config(), RA.CLASSES, dataset_cfg=dict(current_label_method="unlabeled"), device=dev, resident=True)
        kernel = []
        np.random.seed(1)
        for it in range(args.warmup + args.repeats):
            pending = A.PointOps(dev_frames[it % 3])
            d = dict(points=pending, gt_boxes=np.zeros((0, 7), np.float32), gt_names=np.zeros((0,), dtype=str))
            for step in aug.data_augmentor_queue:
                d = step(data_dict=d)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            pending.run(PCR)
            ev[1].record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                kernel.append(ev[0].elapsed_time(ev[1]))
        out["kernel_ms"] = round(float(np.median(kernel)), 3)
        with RA.host_kernels() as H:
            cpu_frames = [torch.from_numpy(f) for f in host_frames]
            out["restatement_ms"], _, _ = time_prepare(H, root, cpu_frames, "cpu", False, 1, args.host_repeats, lambda: None)

    # database creation: one sweep, boxes on a ring
    rng = np.random.default_rng(9)
    infos = []
    for k in range(1):
        boxes, cls, ids = [], [], []
        for c in RA.CLASSES:
            l, w, h, _ = SIZES[c]
            for j in range(args.db_boxes):
                r, a = rng.uniform(8, 50), rng.uniform(-np.pi, np.pi)
                boxes.append([r * np.cos(a), r * np.sin(a), h / 2, l, w, h, rng.uniform(-np.pi, np.pi)])
                cls.append(c)
                ids.append(len(ids))
        infos.append(dict(point_cloud=dict(lidar_sequence="seg", sample_idx=k), pose=np.eye(4), outline_box=np.array(boxes),
                          outline_ids=np.array(ids), outline_cls=np.array(cls)))
    sweeps = [waymo_cloud(50, 160000)]                  # frame 0: every class is written
    db = {}
    for name, fn in (("device", lambda root: A.create_track_groundtruth_database(infos, root, root, RA.CLASSES,
                                                                                   get_lidar=lambda s, i: sweeps[i], device=dev)),
                     ("restatement", lambda root: RA.create_database(infos, root, RA.CLASSES, lambda s, i: sweeps[i].copy()))):
        times = []
        for it in range(1 + (args.repeats if name == "device" else args.host_repeats)):
            with tempfile.TemporaryDirectory() as root:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = fn(root)
                torch.cuda.synchronize()
                if it:
                    times.append(time.perf_counter() - t0)
        db[name + "_ms_per_frame"] = round(float(np.median(times)) * 1e3, 3)
        db["objects_written"] = sum(len(v) for v in res.values())
    db["boxes_per_frame"] = 3 * args.db_boxes
    out["database"] = db
    print(json.dumps(out))


if __name__ == "__main__":
    main()
