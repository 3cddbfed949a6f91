#!/usr/bin/env python3
"""Golden vectors of the BEV-protocol Waymo estimator's host half (tests/golden/waymo_eval2d.npz). Only DATA is written.

The SOURCE of the reference's generate_waymo_type_results, mask_by_distance and limit_period
(cpd/datasets/waymo_unsupervised/waymo_eval2d.py:19-20, 26-85, 170-177) is executed here as it stands, cut out of the file
with ast -- the module itself imports tensorflow and waymo_open_dataset and is never imported. They run on the scene sets
stored in tests/golden/waymo_eval.npz (fresh infos for every call: the reference rewrites them in place). Stored, for
each set (prefix '' = the 40-frame set, 'lg_' = the 6-frame set with raw scores):
  <prefix>pd_<i>, <prefix>gt_fake_<i>, <prefix>gt_plain_<i>, i = 0..5: the six arrays (frame_id, boxes, obj_type, score,
    overlap_nlz, difficulty) for is_gt False, and is_gt True with fake_gt_infos True / False;
  <prefix>pd_near_<i>, i = 0..4 and <prefix>gt_near_<i>, i = 0..4: mask_by_distance(50, boxes, frame_id, obj_type, score,
    overlap_nlz | difficulty) of the prediction arrays and of the fake-lidar ground-truth arrays.
The metric op is outside the reference tree, so nothing of the evaluation itself is stored.
Usage:  python tests/golden/make_waymo_eval2d_golden.py
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np

REF = os.environ.get("CPD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import ref_waymo_eval as R  # noqa: E402


def load_reference():
    """(self stand-in, generate_waymo_type_results, mask_by_distance) executed from the reference file's source."""
    path = os.path.join(REF, "cpd", "datasets", "waymo_unsupervised", "waymo_eval2d.py")
    src = open(path).read()
    tree = ast.parse(src)
    ns = {"np": np}
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "OpenPCDetWaymoDetectionMetricsEstimator"][0]
    fns = {n.name: n for n in tree.body + cls.body if isinstance(n, ast.FunctionDef)}
    for name in ("limit_period", "generate_waymo_type_results", "mask_by_distance"):
        exec(textwrap.dedent(ast.get_source_segment(src, fns[name])), ns)
    classes = [n for n in cls.body if isinstance(n, ast.Assign) and n.targets[0].id == "WAYMO_CLASSES"][0]
    this = types.SimpleNamespace(WAYMO_CLASSES=ast.literal_eval(classes.value))
    return this, ns["generate_waymo_type_results"], ns["mask_by_distance"]


def main():
    this, generate, mask = load_reference()
    z = np.load(os.path.join(HERE, "waymo_eval.npz"))
    classes = [str(c) for c in z["class_names"]]
    out = {}
    for prefix in ("", "lg_"):
        pd = generate(this, R.infos_from_flat(z, prefix)[0], classes, is_gt=False)
        gt_fake = generate(this, R.infos_from_flat(z, prefix)[1], classes, is_gt=True, fake_gt_infos=True)
        gt_plain = generate(this, R.infos_from_flat(z, prefix)[1], classes, is_gt=True, fake_gt_infos=False)
        for tag, arrays in (("pd", pd), ("gt_fake", gt_fake), ("gt_plain", gt_plain)):
            assert len(arrays) == 6 and arrays[1].shape[1] == 5
            for i, a in enumerate(arrays):
                out["%s%s_%d" % (prefix, tag, i)] = np.asarray(a)
        near_pd = mask(this, 50, pd[1], pd[0], pd[2], pd[3], pd[4])
        near_gt = mask(this, 50, gt_fake[1], gt_fake[0], gt_fake[2], gt_fake[3], gt_fake[5])
        assert 0 < len(near_pd[0]) < len(pd[1]) and 0 < len(near_gt[0]) < len(gt_fake[1])
        for tag, arrays in (("pd_near", near_pd), ("gt_near", near_gt)):
            for i, a in enumerate(arrays):
                out["%s%s_%d" % (prefix, tag, i)] = np.asarray(a)
        print("set '%s': %d predictions (%d within 50 m), %d ground truths (%d within 50 m)"
              % (prefix, len(pd[1]), len(near_pd[0]), len(gt_fake[1]), len(near_gt[0])))
    path = os.path.join(HERE, "waymo_eval2d.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
