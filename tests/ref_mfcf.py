"""Plain numpy restatement of the per-frame half of CPD's MFCF generator (cpd/unsupervised_core/mfcf.py:46-80 with
outline_utils.py points_rigid_transform l.328, voxel_sampling l.368, OutlineFitter.box_fit_DGD l.848 and correct_heading l.444),
as cpd_amd.mfcf computes it, on top of tests/ref_outline.py (ground removal, DBSCAN, box_fit with the closed hull)
and tests/ref_cproto_refine.py (density_guided_drift, correct_orientation with the closed-form float32 inverse). No scipy or
sklearn: the GPU tests import it.

Where it departs from the letter of the reference, on purpose: what ref_outline.py and ref_cproto_refine.py already state, and
for correct_heading the same closed-form inverse; its z row is (0, 0, 1, -z) with z rounded to float32.
make_golden_mfcf.py flags the boxes where any of that moves the result by more than 1e-9."""
import numpy as np

import ref_cproto as RC
import ref_cproto_refine as RR
import ref_outline as RO

BIT_DRIFT_X, BIT_DRIFT_Y, BIT_ORIENT_X, BIT_ORIENT_MAX, BIT_TURNED, BIT_FLIPPED = 1, 2, 4, 8, 16, 32
HEAD_PARTS = 10


def window(i, frame_num, frame_interval, n_frames):
    """mfcf.py:53-57 where every frame 0 .. n_frames - 1 has its file."""
    return [j for j in range(i - frame_num, i + frame_num, frame_interval) if 0 <= j < n_frames]


def gather(frames, scores, poses, i, js, thresh):
    """mfcf.py:53-72: the window's rows with H > thresh in frame i's coordinates, then frame i's own rows -> float32 [n, 3]."""
    pts = np.concatenate([RC.points_rigid_transform(frames[j][:, 0:3], poses[j]) for j in js])
    pts = RC.points_rigid_transform(pts, np.linalg.inv(poses[i]))
    keep = np.concatenate([scores[j] for j in js]) > thresh
    return np.concatenate([pts[keep], frames[i][:, 0:3]])


def floor_divide32(a, b):
    """numpy's float32 floor_divide for a >= 0, b > 0, written out (npy_divmodf): the quotient of the fmod-reduced numerator,
    floored, plus one where it sits more than half above its floor."""
    a, b = np.asarray(a, np.float32), np.float32(b)
    mod = np.fmod(a, b)
    div = (a - mod) / b
    fl = np.floor(div)
    fl = np.where(div - fl > np.float32(0.5), fl + np.float32(1.0), fl)
    return np.where(div == 0, np.float32(0.0), fl).astype(np.float32)


def voxel_sampling(points, res=0.1, return_index=False):
    """outline_utils.py:368-389 on float32 rows: cells in the order of their first row, each with its last row."""
    points = np.asarray(points)
    assert points.dtype == np.float32
    cell = np.stack([floor_divide32(points[:, d] - points[:, d].min(), res) for d in range(3)], -1).astype(np.int64)
    assert cell.min() >= 0 and cell.max() < 1 << 21
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    last = np.zeros(len(first), np.int64)
    np.maximum.at(last, inverse.reshape(-1), np.arange(len(points)))
    order = np.argsort(first, kind="stable")
    idx = last[order]
    return (points[idx], idx) if return_index else points[idx]


def correct_heading(points, box, info=None):
    """outline_utils.py:444-485 for one cluster and one box [7] (a copy)."""
    box = np.array(box, np.float64)
    p = np.asarray(points, np.float64)
    X, _ = RC.box_frame_xy(p, RC.inv_rows32(box))
    Z = ((p[:, 0] * 0.0 + p[:, 1] * 0.0) + p[:, 2] * 1.0) + (-np.float64(np.float32(box[2])))
    l = box[3]
    delta_l = l / HEAD_PARTS
    z_x_max, z_x_min = [], []
    for i in range(HEAD_PARTS):
        mask = (-l / 2 + i * delta_l <= X) & (X < -l / 2 + (i + 1) * delta_l)
        if -l / 2 + i * delta_l < 0 and mask.any():
            z_x_min.append(np.max(Z[mask]))
        if -l / 2 + (i + 1) * delta_l > 0 and mask.any():
            z_x_max.append(np.max(Z[mask]))
    if len(z_x_max) == 0:
        z_x_max.append(0)
    if len(z_x_min) == 0:
        z_x_min.append(0)
    flipped = bool(np.mean(z_x_min) < np.mean(z_x_max))
    if info is not None:
        info.update(flipped=flipped, n_min=len(z_x_min), n_max=len(z_x_max))
    if flipped:
        box[6] += np.pi
    return box


def dgd(points, box):
    """box_fit_DGD's tail (l.881-883) on the filtered rows of one cluster: (box, branch bits)."""
    t = RR.stats(*RC.box_frame_xy(points, RC.inv_rows32(box)))
    bits = (BIT_DRIFT_X if t["pos_x"] / t["n"] > 1 / 2 else 0) | (BIT_DRIFT_Y if t["pos_y"] / t["n"] > 1 / 2 else 0)
    box = RR.density_guided_drift(points, box)
    info = {}
    box = RR.correct_orientation(points, box, info=info)
    bits |= (BIT_ORIENT_X if info["branch"] == 'x' else 0) | (BIT_ORIENT_MAX if info["side"] == 'max' else 0)
    bits |= BIT_TURNED if len(info["top"]) > 0 and len(info["bot"]) > 0 else 0
    head = {}
    box = correct_heading(points, box, head)
    bits |= BIT_FLIPPED if head["flipped"] else 0
    return box, bits


def box_fit_dgd(clusters, cfg, offset=0.2, return_bits=False):
    """OutlineFitter.box_fit_DGD (closed hull): [K, 7] float64 (or [] like the reference), the branch bits per box."""
    boxes, idx = RO.box_fit(clusters, cfg, offset, return_index=True)
    out, bits = [], []
    for b, i in zip(boxes, idx):
        pts = clusters[i]
        pts = pts[pts[:, 2] > (pts[:, 2].min() + offset)]
        nb, bt = dgd(pts, b)
        out.append(nb)
        bits.append(bt)
    out = np.array(out) if out else []
    return (out, np.array(bits, np.int32)) if return_bits else out


def frame_boxes(points, cfg, stages=False):
    """mfcf.py:73-77 on the aggregated float32 rows: voxel_sampling, remove_ground, clustering, box_fit_DGD."""
    vox = voxel_sampling(np.ascontiguousarray(points, np.float32))
    xyz = RO.remove_ground(vox, cfg)
    clusters, _ = RO.clustering(xyz, cfg)
    boxes, bits = box_fit_dgd(clusters, cfg, return_bits=True)
    return (boxes, bits, vox) if stages else boxes


def sequence_boxes(frames, scores, poses, cfg, stages=False):
    """mfcf.py:46-80: per frame the boxes (and with stages the bits and the voxel-sampled rows)."""
    g = RO.cfg_get
    out = []
    for i in range(len(frames)):
        js = window(i, g(cfg, "frame_num"), g(cfg, "frame_interval"), len(frames))
        out.append(frame_boxes(gather(frames, scores, poses, i, js, g(cfg, "ppscore_thresh")), cfg, stages))
    return out
