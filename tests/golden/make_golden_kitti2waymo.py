#!/usr/bin/env python3
"""Golden vectors of the KITTI transfer-evaluation path (tests/golden/kitti2waymo.npz). Only DATA is written.

What runs here is the reference's own text. cpd/utils/calibration_kitti.py and cpd/utils/box_utils.py are loaded by file path under
the synthetic package `r` of make_golden.py. Kitti2WaymoDataset does not import (its package pulls the whole dataset stack), so the
point stage of __getitem__ (cpd/datasets/kitti/kitti2waymo_dataset.py, `if self.dataset_cfg.FOV_POINTS_ONLY:` .. `points[:,3:]=0`),
get_fov_flag, generate_prediction_dicts, and the camera block of DetectionsMerger.merge
(cpd/datasets/kitti/kitti_object_eval_python/merge_detections.py, `det_boxes[:,2]+=det_boxes[:,5]/2` .. `['rotation_y'] = ...`) are
read from their files at maker time and executed on stand-ins: the text is never stored.

Content.
  calib<i>_text / calibN_text: calib files of the three calibrations of tests/ref_kitti2waymo.py (two real-shaped, one exact: axis
    permutation V2C, identity R0, integer P2) and calibration 0 without its R0_rect line; <name>_P2 / _R0 / _V2C as the reference
    parses them, and lidar_to_rect / rect_to_img / rect_to_lidar of probe_xyz through the reference object.
  fov_*: three frames of points all round the sensor, one per calibration (image shapes 375x1242, 370x1224, 370x1224): fov_points
    [n, 4], fov_n [3], fov_frames [3, 26], the reference's fov_flag [n], its shifted float64 z of the kept points fov_out_z, the
    number of columns it ends with, and fov_band [n]: reference u or v within 1e-2 px of a border, or |depth| < 1e-3.
  exp_*: the export frames `main` (calibration 0: labels 1 / 2 / 3, a box beyond 60 m, one dropped by the length filter, the exact
    tie of the centre shift, boxes cut by each image border, one wholly outside), `second` (calibration 1), `emptied` (every box
    dropped by the filter), `none` (no box), `exact` (calibration 2) and `straddle` (boxes across the camera plane): inputs
    exp_boxes / exp_scores / exp_labels with exp_n, exp_frames; the reference's annos concatenated (exp_out_<key> with exp_out_n),
    the kept input rows exp_keep, the txt files exp_txt. cam_*: frames main / second / exact through merge's camera block.
  tol_<key>: the largest distance, over all export and camera cases but `straddle`, between the reference's output and the float64
    restatement of the same formulas (ref_kitti2waymo.export_host(ft=np.float64)); tol_bbox includes `straddle`.
  numpy_version: scalar promotion of `weight * 0.3` differs between numpy 1 and 2; the restatement and the kernel follow numpy 2.

Asserted here (conditions of the exact comparisons; inputs are drawn until they hold):
  at most 0.1 % of the points lie in the band, and the float32 restatement's flags equal the reference's on every point;
  every box has |l - 0.2 - 5| >= 1e-3; every class-1 box has |dis1 - dis2| >= 1e-3 except the one exact tie (centre at x = 0, yaw 0);
  no corner has |rect_z| < 0.5 m except in `straddle`; the restatement's keep lists equal the reference's.
Measured with numpy 2.2.6 (metres, radians, pixels): boxes_lidar 3.3e-06, location 5.0e-06, dimensions 1.9e-07, rotation_y 1.6e-07,
alpha 3.7e-07, bbox 1.1e-04. The tests allow 4 x these.
Usage:  python tests/golden/make_golden_kitti2waymo.py
"""
import copy
import os
import pathlib
import re
import sys
import tempfile
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
import ref_kitti2waymo as R  # noqa: E402

DATASET = "cpd/datasets/kitti/kitti2waymo_dataset.py"
MERGER = "cpd/datasets/kitti/kitti_object_eval_python/merge_detections.py"
KEYS = ("boxes_lidar", "location", "dimensions", "rotation_y", "alpha", "bbox")


def load_reference():
    for p in ["r", "r.utils", "r.ops", "r.ops.roiaware_pool3d"]:
        MG._pkg(p)
    stub = types.ModuleType("r.ops.roiaware_pool3d.roiaware_pool3d_utils")
    sys.modules[stub.__name__] = stub
    sys.modules["r.ops.roiaware_pool3d"].roiaware_pool3d_utils = stub
    MG._load("r.utils.common_utils", "cpd/utils/common_utils.py")
    calibration = MG._load("r.utils.calibration_kitti", "cpd/utils/calibration_kitti.py")
    box_utils = MG._load("r.utils.box_utils", "cpd/utils/box_utils.py")
    text = open(os.path.join(MG.REF, DATASET)).read()
    ns = {"np": np, "copy": copy, "box_utils": box_utils}
    for name in ("get_fov_flag", "generate_prediction_dicts"):
        m = re.search(r"^(    def %s\(.*?)(?=^    (?:def |@))" % name, text, re.S | re.M)
        exec(textwrap.dedent(m.group(1)), ns)
    stage = re.search(r"^(        if self\.dataset_cfg\.FOV_POINTS_ONLY:.*?^        points\[:,3:\]=0\n)", text, re.S | re.M).group(1)
    camera = re.search(r"^(            det_boxes\[:,2\]\+=det_boxes\[:,5\]/2.*?\['rotation_y'\] = [^\n]*\n)",
                       open(os.path.join(MG.REF, MERGER)).read(), re.S | re.M).group(1)
    return calibration, box_utils, ns, compile(textwrap.dedent(stage), "point_stage", "exec"), compile(textwrap.dedent(camera), "camera_block", "exec")


def point_stage(code, ns, points, calib, img_shape):
    me = types.SimpleNamespace(dataset_cfg=MG.AttrDict(FOV_POINTS_ONLY=True), get_fov_flag=ns["get_fov_flag"])
    env = {"np": np, "self": me, "points": points.copy(), "calib": calib, "img_shape": img_shape}
    exec(code, env)
    return env["fov_flag"], env["points"], env["pts_rect"]


def camera_block(code, box_utils, boxes, calib, shape):
    me = types.SimpleNamespace(calib_info=[calib], image_info=[shape])
    env = {"np": np, "self": me, "det_boxes": boxes.copy(), "index": 0, "out_infos": [{}], "box_utils": box_utils}
    exec(code, env)
    out = env["out_infos"][0]
    out["boxes_lidar"] = env["det_boxes"]
    return out


def first_good(what, make):
    for seed in range(20261201, 20261201 + 400):
        try:
            got = make(np.random.default_rng(seed))
        except AssertionError as e:
            print("%s: seed %d rejected: %s" % (what, seed, e))
            continue
        print("%s: seed %d" % (what, seed))
        return got
    raise RuntimeError("%s: no seed meets the conditions" % what)


def special_boxes():
    """the named boxes of frame `main` (sensor-height frame, calibration 0, 375 x 1242): (box, label)"""
    z = -0.9 + 1.55
    return [([65.0, 4.0, z, 4.5, 1.9, 1.6, 0.3], 1),        # beyond 60 m: the clamp
            ([20.0, -3.0, z, 5.6, 2.1, 1.8, 1.0], 1),       # dropped by the length filter
            ([0.0, 6.0, z, 4.0, 1.8, 1.5, 0.0], 1),         # the exact tie of the centre shift
            ([10.0, 8.4, z, 4.2, 1.8, 1.5, 0.4], 1),        # cut by the left border
            ([10.0, -8.7, z, 4.2, 1.8, 1.5, -0.4], 2),      # cut by the right border
            ([8.0, 1.0, 1.9 + 1.55, 1.0, 0.8, 1.8, 0.2], 2),   # cut by the top border
            ([5.5, -0.5, z, 4.0, 1.8, 1.5, 0.1], 3),        # cut by the bottom border
            ([5.0, 30.0, z, 4.2, 1.8, 1.5, 2.0], 1)]        # wholly outside the image


def main():
    calibration, box_utils, ns, stage_code, camera_code = load_reference()
    out = {"numpy_version": np.array(np.__version__), "classes": np.array(R.CLASSES)}
    assert int(np.__version__.split(".")[0]) >= 2, "the restatement follows numpy 2 scalar promotion"
    tmp = pathlib.Path(tempfile.mkdtemp())

    # ---- calibrations
    probe = np.random.default_rng(7).uniform(-40, 40, (16, 3)).astype(np.float32)
    out["probe_xyz"] = probe
    calibs = []
    for name, text in [("calib%d" % i, R.calib_text(i)) for i in range(3)] + [("calibN", R.calib_text(0, r0=False))]:
        (tmp / "c.txt").write_text(text)
        c = calibration.Calibration(tmp / "c.txt")
        out[name + "_text"] = np.array(text)
        out[name + "_P2"], out[name + "_R0"], out[name + "_V2C"] = c.P2, c.R0, c.V2C
        out[name + "_rect"] = c.lidar_to_rect(probe)
        img, depth = c.rect_to_img(probe + np.float32([0, 0, 45]))
        out[name + "_img"], out[name + "_depth"] = img, depth
        out[name + "_lidar"] = c.rect_to_lidar(probe)
        calibs.append(c)
    assert out["calibN_R0"].dtype == np.float64 and out["calib0_R0"].dtype == np.float32
    calibs = calibs[:3]
    records = np.stack([R.frame_record(c, s) for c, s in zip(calibs, R.IMAGE_SHAPES)])

    # ---- the point stage
    def fov_case(rng):
        frames = [R.gen_points(rng, n) for n in (5200, 5000, 4800)]
        flags, zs, bands = [], [], []
        for pts, c, shape, rec in zip(frames, calibs, R.IMAGE_SHAPES, records):
            flag, after, _ = point_stage(stage_code, ns, pts, c, np.array(shape, np.int32))
            pts_img, depth = c.rect_to_img(c.lidar_to_rect(pts[:, 0:3]))
            band = np.zeros(len(pts), bool)
            for col, hi in ((0, shape[1]), (1, shape[0])):
                band |= (np.abs(pts_img[:, col]) < 1e-2) | (np.abs(pts_img[:, col] - hi) < 1e-2)
            band |= np.abs(depth) < 1e-3
            assert band.mean() <= 1e-3, "more than 0.1 %% of the points in the band"
            assert np.array_equal(R.fov_flag(pts[:, :3], rec), flag), "the float32 restatement decides a point differently"
            assert np.array_equal(R.fov_flag(pts[:, :3], rec, np.float64)[~band], flag[~band])
            assert after.dtype == np.float64 and after.shape[1] == 6 and not after[:, 3:].any()
            assert np.array_equal(after[:, :2], pts[flag][:, :2]) and 0.15 < flag.mean() < 0.35
            flags.append(flag), zs.append(after[:, 2]), bands.append(band)
        return frames, flags, zs, bands

    frames, flags, zs, bands = first_good("fov", fov_case)
    out["fov_points"], out["fov_n"] = np.concatenate(frames), np.array([len(f) for f in frames], np.int32)
    out["fov_frames"], out["fov_flag"], out["fov_band"] = records, np.concatenate(flags), np.concatenate(bands)
    out["fov_out_z"], out["fov_ref_cols"] = np.concatenate(zs), np.int32(6)

    # ---- the export
    def run_reference(boxes, scores, labels, n, which):
        at = np.concatenate([[0], np.cumsum(n)])
        pred = [{"pred_boxes": torch.from_numpy(boxes[a:b].copy()), "pred_scores": torch.from_numpy(scores[a:b].copy()),
                 "pred_labels": torch.from_numpy(labels[a:b].copy())} for a, b in zip(at[:-1], at[1:])]
        batch = {"frame_id": ["%06d" % i for i in range(len(n))], "calib": [calibs[w] for w in which],
                 "image_shape": [np.array(R.IMAGE_SHAPES[w], np.int32) for w in which]}
        annos = ns["generate_prediction_dicts"](batch, pred, R.CLASSES, tmp)
        return annos, [(tmp / ("%s.txt" % f)).read_text() for f in batch["frame_id"]]

    def export_case(rng):
        sb = special_boxes()
        b0, s0, l0 = R.gen_boxes(rng, 36)
        b0 = np.concatenate([b0, np.array([b for b, _ in sb], np.float32)])
        l0 = np.concatenate([l0, np.array([l for _, l in sb], np.int64)])
        s0 = np.sort(rng.uniform(0.1, 0.95, len(b0)))[::-1].astype(np.float32)
        order = rng.permutation(len(b0))
        b0, l0 = b0[order], l0[order]
        b1, s1, l1 = R.gen_boxes(rng, 30)
        b2, s2, l2 = R.gen_boxes(rng, 5)
        b2[:, 3] = rng.uniform(5.4, 7.0, 5)                                    # `emptied`
        b4, s4, l4 = R.gen_boxes(rng, 12)
        b5 = np.array([[0.5, 3.0, 0.65, 4.0, 1.8, 1.5, 0.1], [1.0, -2.0, 0.65, 4.4, 1.9, 1.6, 0.7], [12.0, 1.0, 0.65, 4.0, 1.8, 1.5, 0.5]], np.float32)
        s5, l5 = np.float32([0.9, 0.8, 0.7]), np.int64([1, 2, 1])
        n = np.array([len(b0), len(b1), len(b2), 0, len(b4), len(b5)], np.int32)
        which = [0, 1, 0, 1, 2, 0]
        boxes, scores, labels = np.concatenate([b0, b1, b2, b4, b5]), np.concatenate([s0, s1, s2, s4, s5]), np.concatenate([l0, l1, l2, l4, l5])
        annos, txt = run_reference(boxes, scores, labels, n, which)
        at = np.concatenate([[0], np.cumsum(n)])
        keeps = []
        for f, (a, b) in enumerate(zip(at[:-1], at[1:])):
            got = R.export_frame(boxes[a:b], scores[a:b], labels[a:b], records[which[f]], R.MODE_PREDICT)
            assert (np.abs(got["length"] - 5) >= 1e-3).all(), "a length within 1e-3 of the filter"
            tie = np.abs(got["dis"]) < 1e-3
            assert tie.sum() == (1 if f == 0 else 0), "%d centre shifts within 1e-3 of a tie in frame %d" % (tie.sum(), f)
            assert (got["dis"][tie] == 0).all(), "the tie is not exact"
            if f != 5:
                assert (np.abs(got["rect_z"]) >= 0.5).all(), "a corner within 0.5 m of the camera plane"
            else:
                assert (np.abs(got["rect_z"]) >= 0.2).all() and (got["rect_z"] < 0).any() and (got["rect_z"] > 0).any()
            assert len(got["keep"]) == len(annos[f]["score"]), "the restatement keeps other boxes than the reference"
            assert np.array_equal(got["score"], annos[f]["score"]) if len(got["keep"]) else True
            keeps.append(got["keep"])
        a0 = annos[0]
        assert len(a0["score"]) == n[0] - 1 and len(annos[2]["score"]) == 0 and len(annos[3]["score"]) == 0
        assert set(a0["name"]) == set(R.CLASSES)
        w, h = R.IMAGE_SHAPES[0][1] - 1, R.IMAGE_SHAPES[0][0] - 1
        inside = lambda v, hi: (v > 0) & (v < hi)
        bb = a0["bbox"]
        assert ((bb[:, 0] == 0) & inside(bb[:, 2], w)).any() and ((bb[:, 2] == w) & inside(bb[:, 0], w)).any(), "no box cut left / right"
        assert ((bb[:, 1] == 0) & inside(bb[:, 3], h)).any() and ((bb[:, 3] == h) & inside(bb[:, 1], h)).any(), "no box cut top / bottom"
        assert ((bb[:, 0] == bb[:, 2]) & (bb[:, 0] == 0)).any(), "no box wholly outside"
        return boxes, scores, labels, n, which, annos, txt, keeps

    boxes, scores, labels, n, which, annos, txt, keeps = first_good("export", export_case)
    out["exp_boxes"], out["exp_scores"], out["exp_labels"], out["exp_n"] = boxes, scores, labels, n
    out["exp_frames"], out["exp_names"] = records[which], np.array(["main", "second", "emptied", "none", "exact", "straddle"])
    out["exp_out_n"] = np.array([len(a["score"]) for a in annos], np.int32)
    out["exp_keep"] = np.concatenate(keeps).astype(np.int32)
    out["exp_txt"] = np.array(txt)
    full = [a for a in annos if len(a["score"])]
    for key in ("name", "score", "truncated", "occluded") + KEYS:
        out["exp_out_" + key] = np.concatenate([a[key] for a in full])
        assert key == "name" or out["exp_out_" + key].dtype == (np.float64 if key in ("truncated", "occluded") else np.float32)
    empty = annos[3]
    assert all(empty[k].dtype == np.float64 and not empty[k].any() for k in ("name", "alpha", "bbox", "boxes_lidar", "score"))

    # ---- merge's camera block on frames main / second / exact (the boxes lowered to the KITTI sensor)
    at = np.concatenate([[0], np.cumsum(n)])
    cam_frames = [0, 1, 4]
    cam_in, cam_out = [], []
    for f in cam_frames:
        b = boxes[at[f]:at[f + 1]].copy()
        b[:, 2] -= np.float32(1.55)
        b = b[np.abs(b[:, 0]) > 4]                       # (the tie box sits across the camera plane)
        cam_in.append(b)
        cam_out.append(camera_block(camera_code, box_utils, b, calibs[which[f]], np.array(R.IMAGE_SHAPES[which[f]], np.int32)))
    out["cam_boxes"], out["cam_n"] = np.concatenate(cam_in), np.array([len(b) for b in cam_in], np.int32)
    out["cam_frames"] = records[[which[f] for f in cam_frames]]
    for key in KEYS:
        out["cam_out_" + key] = np.concatenate([c[key] for c in cam_out])

    # ---- tolerances: reference against the float64 restatement, per key
    tol = dict.fromkeys(KEYS, 0.0)

    def measure(ref, wide, keys):
        for key in keys:
            got = {"location": wide["camera"][:, 0:3], "dimensions": wide["camera"][:, 3:6], "rotation_y": wide["camera"][:, 6]}.get(key, wide.get(key))
            d = np.abs(np.asarray(ref[key], np.float64).reshape(got.shape) - got)
            tol[key] = max(tol[key], float(d.max(initial=0.0)))

    for f in range(len(n)):
        if out["exp_out_n"][f]:
            wide = R.export_frame(boxes[at[f]:at[f + 1]], scores[at[f]:at[f + 1]], labels[at[f]:at[f + 1]], records[which[f]], R.MODE_PREDICT, np.float64)
            measure(annos[f], wide, KEYS if f != 5 else ("bbox",))
    for b, c, f in zip(cam_in, cam_out, cam_frames):
        b = b.copy()
        b[:, 2] += b[:, 5] / 2
        measure(c, R.export_frame(b, None, None, records[which[f]], R.MODE_CAMERA, np.float64), KEYS)
    for key in KEYS:
        out["tol_" + key] = np.float64(tol[key])
        assert tol[key] > 0
    path = os.path.join(HERE, "kitti2waymo.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size < 300 * 1024
    print("kept points", [int(f.sum()) for f in flags], "in the band", int(out["fov_band"].sum()))
    print("export kept", out["exp_out_n"].tolist(), "of", n.tolist())
    print("tolerances", {k: "%.2g" % v for k, v in tol.items()})


if __name__ == "__main__":
    main()
