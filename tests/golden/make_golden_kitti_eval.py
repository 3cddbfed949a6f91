#!/usr/bin/env python3
"""Golden vectors of the KITTI-protocol evaluation, computed by the REFERENCE itself (build container only).

cpd/datasets/kitti/kitti_object_eval_python/{eval.py, rotate_iou.py} are imported by file path under a synthetic
package, with `numba` replaced by a stand-in module: `jit` is the identity (both decorator forms), `numba.cuda.jit` is
the identity, and `cuda.local.array` is `np.zeros`, so every jitted function runs as plain Python / numpy. The numba.cuda
launcher cannot run, so rotate_iou_gpu_eval is computed the way its kernel does it: devRotateIoUEval(query_box, box,
criterion) per pair (rotate_iou.py:289-291). A pair whose intersection overflows the reference's 8-point buffer raises
IndexError under the stand-in; such pairs are dropped from the box sets (rot_valid = 0) and re-jittered in the dataset.

Only DATA is written (tests/golden/kitti_eval.npz):
  * rot_boxes [N, 5], rot_query [K, 5] and rot_iou_<c> [N, K] for criterion c in -1 / 0 / 1 / 2 (rot_valid [N, K]);
  * a seeded synthetic KITTI-format set (cpd_amd.synthetic.kitti_annos, 100 frames; gt_* / dt_* flat arrays with
    gt_num / dt_num per frame), detections re-jittered until no overlap lies within 1e-4 of 0.25 / 0.5 / 0.7;
  * get_official_eval_result(gt, dt, ['Car', 'Pedestrian', 'Cyclist'], PR_detail_dict): pr_<key> arrays, the
    ret_dict as ret_keys / ret_values, and the result string.
Usage:  python tests/golden/make_golden_kitti_eval.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

REF = os.environ.get("CPD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
EVAL_DIR = os.path.join(REF, "cpd", "datasets", "kitti", "kitti_object_eval_python")


def _numba_standin():
    def jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f

    numba = types.ModuleType("numba")
    cuda = types.ModuleType("numba.cuda")
    numba.jit = jit
    numba.float32 = np.float32
    cuda.jit = jit
    cuda.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype=dtype))
    numba.cuda = cuda
    return numba, cuda


def load_reference():
    numba, cuda = _numba_standin()
    sys.modules["numba"], sys.modules["numba.cuda"] = numba, cuda
    pkg = types.ModuleType("kref")
    pkg.__path__ = [EVAL_DIR]
    sys.modules["kref"] = pkg
    mods = {}
    for name in ("rotate_iou", "eval"):
        spec = importlib.util.spec_from_file_location("kref." + name, os.path.join(EVAL_DIR, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["kref." + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["rotate_iou"], mods["eval"]


RI, EV = load_reference()


def ref_rotate_iou(boxes, query_boxes, criterion=-1, device_id=0):
    """rotate_iou_gpu_eval's kernel, pair by pair: iou[n, k] = devRotateIoUEval(query[k], boxes[n]); NaN = overflow."""
    boxes = np.asarray(boxes).astype(np.float32)
    query_boxes = np.asarray(query_boxes).astype(np.float32)
    iou = np.zeros((boxes.shape[0], query_boxes.shape[0]), dtype=np.float32)
    for n in range(boxes.shape[0]):
        for k in range(query_boxes.shape[0]):
            try:
                iou[n, k] = RI.devRotateIoUEval(query_boxes[k].copy(), boxes[n].copy(), criterion)
            except IndexError:
                iou[n, k] = np.nan
    return iou


EV.rotate_iou_gpu_eval = ref_rotate_iou


def rot_box_sets(rng):
    """Hand-placed pairs (touching, near-touching, containment, 0 / 90 / 180 degrees, small angles, a tiny box in a big
    one) followed by random boxes; dims stay below ~1.6 so raw areas keep float32 steps under 1e-6."""
    q = [[0, 0, 1.0, 0.5, 0], [0, 0, 1.0, 0.5, np.pi / 2], [0, 0, 1.0, 0.5, np.pi], [0, 0, 1.5, 1.5, 0.01],
         [0.3, -0.2, 0.05, 0.04, 0.3], [2.0, 2.0, 0.8, 0.6, -0.7], [0, 0, 1.2, 0.4, 1e-3]]
    b = [[0, 0, 1.0, 0.5, 0], [1.0, 0, 1.0, 0.5, 0], [1.0001, 0, 1.0, 0.5, 0], [0.9999, 0, 1.0, 0.5, 0],
         [0, 0, 0.2, 0.1, 0.5], [0, 0, 1.4, 1.4, 0.02], [0, 0, 1.0, 0.5, np.pi / 2], [0, 0, 1.0, 0.5, -np.pi],
         [0.1, 0.05, 1.0, 0.5, 0.002], [2.1, 1.9, 0.8, 0.6, -0.69], [0.3, -0.2, 1.2, 1.1, 0.0]]
    q += [[*rng.uniform(-1, 1, 2), *rng.uniform(0.1, 1.6, 2), rng.uniform(-np.pi, np.pi)] for _ in range(23)]
    b += [[*rng.uniform(-1, 1, 2), *rng.uniform(0.1, 1.6, 2), rng.uniform(-np.pi, np.pi)] for _ in range(29)]
    return np.array(b, np.float32), np.array(q, np.float32)


def reference_overlap_fns(g, d):
    dc = g["name"] == "DontCare"
    bev = lambda a: np.concatenate([a["location"][:, [0, 2]], a["dimensions"][:, [0, 2]], a["rotation_y"][:, None]], 1)
    d3 = lambda a: np.concatenate([a["location"], a["dimensions"], a["rotation_y"][:, None]], 1)
    return [EV.image_box_overlap(d["bbox"], g["bbox"]), EV.image_box_overlap(d["bbox"], g["bbox"][dc], 0),
            ref_rotate_iou(bev(d), bev(g)), EV.d3_box_overlap(d3(d), d3(g)).astype(np.float64)]


def main():
    import ref_kitti_eval as R
    from cpd_amd.synthetic import kitti_annos

    rng = np.random.default_rng(20261016)
    out = {}
    boxes, query = rot_box_sets(rng)
    valid = np.ones((len(boxes), len(query)), np.int8)
    out["rot_boxes"], out["rot_query"] = boxes, query
    for c in (-1, 0, 1, 2):
        iou = ref_rotate_iou(boxes, query, c)
        valid &= ~np.isnan(iou)
        out["rot_iou_%s" % ("m1" if c == -1 else c)] = iou
    for c in ("m1", "0", "1", "2"):
        out["rot_iou_" + c] = np.where(valid == 1, out["rot_iou_" + c], 0).astype(np.float32)
    out["rot_valid"] = valid

    gt, dt = kitti_annos(100, seed=7)
    R.separate_from_thresholds(gt, dt, reference_overlap_fns, seed=7)
    out.update(R.annos_to_flat(gt, "gt_"))
    out.update(R.annos_to_flat(dt, "dt_"))
    pr_detail = {}
    with contextlib.redirect_stdout(io.StringIO()):      # the reference's debug prints
        result, ret = EV.get_official_eval_result(gt, dt, ["Car", "Pedestrian", "Cyclist"], PR_detail_dict=pr_detail)
    for k, v in pr_detail.items():
        out["pr_" + k] = np.asarray(v, np.float64)
    out["ret_keys"] = np.array(list(ret.keys()))
    out["ret_values"] = np.array([float(v) for v in ret.values()], np.float64)
    out["result"] = np.array(result)
    path = os.path.join(HERE, "kitti_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    print(result)


if __name__ == "__main__":
    main()
