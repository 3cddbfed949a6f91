#!/usr/bin/env python3
"""Golden vectors of the MFCF pseudo-label generator, computed by the REFERENCE itself (build container only).

cpd/unsupervised_core/mfcf.py, outline_utils.py, precompute_ppscore.py and the tracker package are imported from the reference
tree by path, as make_golden_outline.py does (numpy 2 removed np.mat: it is aliased to np.asmatrix first; ground_removal's
argsort is made stable, §5l). The input is cpd_amd.synthetic.ppscore_sequence(SEED): N_FRAMES sweeps of a short drive with
parked and moving boxes and poses with a large origin, generated as float32 with the odd frames stored as float16 (regenerated
from the seed by the tests; a digest is stored). It is written to a temporary directory as the dataset stores a sequence, the H
files are made by the reference's own save_pp_score (PP_MAX_WIN, PP_WIN_INTE), and the reference's whole
MFCF.generate_outline_box runs over it with MFCF_GENERATOR_CONFIG, max_prediction_num lowered to MAX_PREDICTION_NUM so that
tracks die inside the sequence. A second pass feeds the same per-frame boxes to the reference's TrackSmooth with lwh_win_size =
yaw_win_size = SMOOTH_WIN (the yaml's 0 switches the size / yaw smoothing off; OYSTER's config turns it on), and a third pass
feeds it swapped_boxes(): the same boxes with l and w exchanged in every third one.

Two branches the issue lists cannot occur in the reference's own MFCF run, whatever the seed, and are covered elsewhere:
  * correct_orientation's y axis: box_fit's box is the bounding rectangle of the very rows box_fit_DGD passes on, so after the
    drift the cluster spans the whole of l and of w and ((max_x - min_x) / l) * 2 > (max_y - min_y) / w always holds (0 of
    ~200 boxes in each of twelve seeds). The GPU tests force it with a hand-built box through the same kernel.
  * the tracker's l < w swap: box_fit hands out l >= w, the size states have no motion terms, and a Kalman update is a convex
    combination of two such states. The third pass exists to reach it.

Stored (data only): seed, digest, the float16 H arrays; per frame the reference's per-frame boxes (copied before the tracker
sees them), the restatement's branch bits and a flag per box where the restatement (tests/ref_mfcf.py) differs by more than
1e-9; the count and a digest of the voxel-sampled rows; the final outline_box / ids / cls / dif of both tracker passes; the counts
printed below.
Asserted: see the end of main().
Usage:  python tests/golden/make_golden_mfcf.py [seed ...]     (several seeds: the first that meets every condition is kept)
"""
import copy
import hashlib
import os
import pickle
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("CPD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SEED, N_FRAMES, N_AZ = 10, 12, 360
ORIGIN = (4200.0, -1800.0, 35.0)
SEQ = "segment-87654321_mfcf"
PP_MAX_WIN, PP_WIN_INTE = 4, 1
MAX_PREDICTION_NUM = 4
SMOOTH_WIN = 3
OUT = os.path.join(HERE, "mfcf.npz")


def golden_config(smooth=False):
    from cpd_amd.mfcf import MFCF_GENERATOR_CONFIG
    g = copy.deepcopy(MFCF_GENERATOR_CONFIG)
    g["max_prediction_num"] = MAX_PREDICTION_NUM
    if smooth:
        g["lwh_win_size"] = g["yaw_win_size"] = SMOOTH_WIN
    return dict(InitLabelGenerator='MFCF', GeneratorConfig=g)


def namespace(cfg):
    return types.SimpleNamespace(InitLabelGenerator=cfg["InitLabelGenerator"],
                                 GeneratorConfig=types.SimpleNamespace(**cfg["GeneratorConfig"]))


def sequence(seed=SEED, n_frames=N_FRAMES, n_az=N_AZ):
    """(frames, poses): odd frames float16, even frames float32."""
    from cpd_amd import synthetic
    frames, poses = synthetic.ppscore_sequence(seed, n_frames, n_az, np.float32, ORIGIN)
    return [f.astype(np.float16) if k % 2 else f for k, f in enumerate(frames)], poses


def digest(frames, poses):
    h = hashlib.sha256()
    for f, p in zip(frames, poses):
        h.update(np.ascontiguousarray(f).tobytes())
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def rows_digest(rows):
    return hashlib.sha256(np.ascontiguousarray(rows, np.float32).tobytes()).hexdigest()


def write_sequence(root, frames, poses, scores=None, seq=SEQ):
    os.makedirs(os.path.join(root, seq, "ppscore") if scores is not None else os.path.join(root, seq), exist_ok=True)
    for i, f in enumerate(frames):
        np.save(os.path.join(root, seq, "%04d.npy" % i), f)
        if scores is not None:
            np.save(os.path.join(root, seq, "ppscore", "%04d.npy" % i), scores[i])
    with open(os.path.join(root, seq, seq + ".pkl"), "wb") as f:
        pickle.dump([dict(pose=p.copy()) for p in poses], f)


def unpack_infos(z, prefix, poses):
    infos = []
    for i, p in enumerate(poses):
        infos.append(dict(pose=p, outline_box=z["%s%d_box" % (prefix, i)], outline_ids=z["%s%d_ids" % (prefix, i)],
                          outline_cls=z["%s%d_cls" % (prefix, i)], outline_dif=z["%s%d_dif" % (prefix, i)]))
    return infos


def frame_boxes(z, i):
    b = z["pf%d_box" % i]
    return b.copy() if len(b) else []


def swapped_boxes(per_frame):
    """The third pass's input: l and w exchanged in every third box (counted over the sequence), the rest as they are."""
    out, k = [], 0
    for b in per_frame:
        b = np.array(b, np.float64).reshape(-1, 7).copy()
        for r in range(len(b)):
            if k % 3 == 0:
                b[r, 3], b[r, 4] = b[r, 4], b[r, 3]
            k += 1
        out.append(b if len(b) else [])
    return out


class _StableNumpy(types.ModuleType):
    def __init__(self):
        super().__init__("numpy_stable_argsort")

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kw):
        return np.argsort(a, kind="stable")


def run(seed, verbose=True):
    """The reference over the drive of `seed`: (arrays to store, counts, failed conditions)."""
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    import ref_mfcf as RM
    import ref_outline as RO
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import cpd.unsupervised_core.ground_removal as gr
    import cpd.unsupervised_core.outline_utils as ou
    import cpd.unsupervised_core.mfcf as mf
    import cpd.unsupervised_core.precompute_ppscore as pp
    from cpd.unsupervised_core.tracker import trajectory as tj

    cfg = golden_config()
    gcfg = cfg["GeneratorConfig"]
    frames, poses = sequence(seed)
    out = dict(seed=np.array(seed), n_frames=np.array(N_FRAMES), n_az=np.array(N_AZ), seq=np.array(SEQ),
               digest=np.array(digest(frames, poses)), n_points=np.array([len(f) for f in frames], np.int32))
    rec = dict(gathered=[], vox=[], labels=None, swaps=0)
    real_vs, real_ts, real_filtering = ou.voxel_sampling, ou.TrackSmooth, tj.Trajectory.filtering

    def recording_vs(points, *a, **kw):
        rec["gathered"].append(np.array(points))
        res = real_vs(points, *a, **kw)
        rec["vox"].append(np.array(res))
        return res

    class RecordingTrackSmooth(real_ts):
        def tracking(self, all_objects, all_pose, scores=None):
            rec["labels"] = [np.array(b, np.float64).reshape(-1, 7).copy() for b in all_objects]   # before it mutates them
            rec["tracker"] = self
            return super().tracking(all_objects, all_pose, scores)

    def counting_filtering(self, config, pose=None):
        for ob in self.trajectory.values():
            s = ob.updated_state
            if s is not None and s[9, 0] < s[10, 0]:
                rec["swaps"] += 1
        return real_filtering(self, config, pose=pose)

    unstable_np = gr.np
    with tempfile.TemporaryDirectory() as root:
        write_sequence(root, frames, poses)
        assert pp.save_pp_score(SEQ, root, PP_MAX_WIN, PP_WIN_INTE) is True
        scores = [np.load(os.path.join(root, SEQ, "ppscore", "%04d.npy" % i)) for i in range(N_FRAMES)]
        gr.np, mf.voxel_sampling, mf.TrackSmooth, tj.Trajectory.filtering = _StableNumpy(), recording_vs, RecordingTrackSmooth, \
            counting_filtering
        try:
            ref_infos = mf.MFCF(SEQ, root, namespace(cfg))()
        finally:
            gr.np, mf.voxel_sampling, mf.TrackSmooth, tj.Trajectory.filtering = unstable_np, real_vs, real_ts, real_filtering
    for i, h in enumerate(scores):
        assert h.dtype == np.float16 and len(h) == len(frames[i])
        out["h%d" % i] = h

    # the restatement beside the reference, frame by frame
    n_box = n_flag = 0
    branch = np.zeros((6, 2), np.int64)
    for i in range(N_FRAMES):
        js = RM.window(i, gcfg["frame_num"], gcfg["frame_interval"], N_FRAMES)
        g = RM.gather(frames, scores, poses, i, js, gcfg["ppscore_thresh"])
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), rec["gathered"][i].astype(np.float32).view(np.uint32)), \
            "frame %d: the aggregated rows differ from the reference's" % i
        boxes, bits, vox = RM.frame_boxes(g, gcfg, stages=True)
        assert vox.shape == rec["vox"][i].shape and np.array_equal(vox.view(np.uint32), rec["vox"][i].view(np.uint32)), \
            "frame %d: voxel_sampling differs from the reference's" % i
        ref_b = rec["labels"][i]
        assert len(boxes) == len(ref_b), "frame %d: %d boxes, the reference has %d" % (i, len(boxes), len(ref_b))
        boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
        flag = (np.abs(boxes - ref_b).max(1) > 1e-9) if len(ref_b) else np.zeros(0, bool)
        out["pf%d_box" % i], out["pf%d_bits" % i], out["pf%d_flag" % i] = ref_b, np.asarray(bits, np.int32), flag
        out["vox%d_n" % i], out["vox%d_digest" % i] = np.array(len(vox)), np.array(rows_digest(vox))
        n_box += len(ref_b)
        n_flag += int(flag.sum())
        for k in range(6):
            for b in bits:
                branch[k, 1 if b & (1 << k) else 0] += 1
    for i, info in enumerate(ref_infos):
        out["fin%d_box" % i], out["fin%d_ids" % i] = np.asarray(info['outline_box']), np.asarray(info['outline_ids'])
        out["fin%d_cls" % i], out["fin%d_dif" % i] = np.asarray(info['outline_cls']), np.asarray(info['outline_dif'])

    # what the tracker met
    trk = rec["tracker"].tracker
    died_missed = sum(1 for t in trk.dead_trajectories.values() if t.consecutive_missed_num >= MAX_PREDICTION_NUM)
    died_new = sum(1 for t in trk.dead_trajectories.values()
                   if len(t) - t.consecutive_missed_num == 1 and t.consecutive_missed_num < MAX_PREDICTION_NUM)
    interpolated = sum(1 for t in list(trk.dead_trajectories.values()) + list(trk.active_trajectories.values())
                       for k, ob in t.trajectory.items()
                       if t.first_updated_timestamp < k < t.last_updated_timestamp and ob.detected_state is None)
    empty_frames = sum(1 for info in ref_infos if len(info['outline_box']) == 0)

    # the second tracker pass: size / yaw smoothing on
    scfg = golden_config(smooth=True)
    ts = real_ts(namespace(scfg).GeneratorConfig)
    ts.tracking([b.copy() if len(b) else [] for b in rec["labels"]], [p.copy() for p in poses])
    for i in range(N_FRAMES):
        objs, ids, cls, dif = ts.get_current_frame_objects_and_cls(i)
        out["smo%d_box" % i], out["smo%d_ids" % i], out["smo%d_cls" % i], out["smo%d_dif" % i] = objs, ids, cls, dif

    # the third pass: boxes with l < w, which the tracker turns (counted by the patched filtering)
    rec["swaps"] = 0
    tj.Trajectory.filtering = counting_filtering
    try:
        ts = real_ts(namespace(scfg).GeneratorConfig)
        ts.tracking(swapped_boxes(rec["labels"]), [p.copy() for p in poses])
    finally:
        tj.Trajectory.filtering = real_filtering
    for i in range(N_FRAMES):
        objs, ids, cls, dif = ts.get_current_frame_objects_and_cls(i)
        out["swp%d_box" % i], out["swp%d_ids" % i], out["swp%d_cls" % i], out["swp%d_dif" % i] = objs, ids, cls, dif

    counts = dict(boxes=n_box, flagged=n_flag, drift_x=branch[0].tolist(), drift_y=branch[1].tolist(),
                  orient_axis=branch[2].tolist(), orient_side=branch[3].tolist(), turned=branch[4].tolist(),
                  heading=branch[5].tolist(), died_missed=died_missed, died_new=died_new, interpolated=interpolated,
                  swaps=rec["swaps"], empty_frames=empty_frames, tracks=len(trk.dead_trajectories) + len(trk.active_trajectories),
                  final_boxes=sum(len(i['outline_box']) for i in ref_infos))
    failed = []
    if n_box < 40:
        failed.append("fewer than 40 per-frame boxes")
    for name in ("drift_x", "drift_y", "orient_side", "heading"):
        if min(counts[name]) < 3:
            failed.append("%s branch taken %r times" % (name, counts[name]))
    if counts["orient_axis"][1] < 3:
        failed.append("orientation along x taken %d times" % counts["orient_axis"][1])
    if n_flag > 0.10 * n_box:
        failed.append("%d of %d boxes flagged" % (n_flag, n_box))
    for name in ("died_missed", "died_new", "interpolated", "swaps"):
        if counts[name] < 1:
            failed.append("no %s" % name)
    out["counts_keys"] = np.array(sorted(k for k in counts if not isinstance(counts[k], list)))
    out["counts_vals"] = np.array([counts[k] for k in out["counts_keys"]], np.int64)
    out["branch_counts"] = branch
    if verbose:
        print("seed %d: %r" % (seed, counts))
        for f in failed:
            print("   NOT MET:", f)
    return out, counts, failed


def main():
    seeds = [int(a) for a in sys.argv[1:]] or [SEED]
    for seed in seeds:
        out, counts, failed = run(seed)
        if not failed:
            break
    assert not failed, failed
    assert seed == SEED, "set SEED = %d in this file, then run it again" % seed
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
