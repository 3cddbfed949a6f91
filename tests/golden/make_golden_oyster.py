#!/usr/bin/env python3
"""Golden vectors of the OYSTER pseudo-label generator, computed by the REFERENCE itself (build container only).

cpd/unsupervised_core/oyster.py, outline_utils.py, ground_removal.py and the tracker package are imported from the reference
tree by path, as make_golden_mfcf.py does (np.mat aliased to np.asmatrix; ground_removal's argsort made stable, §5l). The
reference's whole OYSTER.generate_outline_box runs twice:

  Run A, the point branch: N_FRAMES_A sweeps of cpd_amd.synthetic.ppscore_sequence(SEED) at N_AZ azimuths (odd frames stored as
  float16), written as the dataset stores a sequence; OYSTER's yaml config with max_prediction_num lowered to
  MAX_PREDICTION_NUM_A and remove_short_track to REMOVE_SHORT_TRACK_A, so that tracks die and short tracks are removed inside
  the drive. Stored: the per-frame raw box_fit boxes (copied before the tracker sees them), a flag per box where the closed-hull
  restatement (tests/ref_outline.py, §5l) differs by more than 1e-9 or make_golden_outline.cluster_flags marks its cluster (the
  open hull, Qhull's vertex set, best scores tied within 1e-9: the rectangle is then the sort's choice), and the final infos.
  Asserted: the restatement's box counts are the reference's in every frame, at most 10 % of the boxes are flagged, at least
  one track dies and one is removed as short.

  Run B, the box branch: box_drive(SEED), a hand-built <seq>_outline_MFCF.pkl of N_FRAMES_B frames whose outline_box rows are
  smooth synthetic trajectories (no point clouds), with OYSTER's yaml config unchanged. The timeline is laid out so that one
  track is alone in the first frames and another in the last ones (a frame's only object is lost: their final lengths are 6 and
  5), one track is longer than 80 entries and one between 60 and 80, one is Dis_Small and one Dis_Large throughout, and the last
  frames hold nothing. Stored: a digest of the input (the tests rebuild it from the seed) and the final infos.

Asserted, over the two runs together (see run()): tracks of final length exactly 5 (dropped) and exactly 6 (kept); one of 80
entries or more and one of 60..79; a frame with exactly one surviving object and one with none; Dis_Small and Dis_Large boxes
dropped; each of the four candidate corners chosen; no two equal distances in a track; the restatement (tests/ref_oyster.py
after cpd_amd.tracker) reproduces both runs' final infos: ids, classes and dif equal, boxes within 1e-9. The counts are printed
and stored.
Usage:  python tests/golden/make_golden_oyster.py [seed ...]     (several seeds: the first that meets every condition is kept)
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
sys.path.insert(0, HERE)

from make_golden_mfcf import _StableNumpy, digest, namespace, write_sequence  # noqa: E402
from make_golden_outline import cluster_flags  # noqa: E402

SEED = 5
N_FRAMES_A, N_AZ = 16, 360
ORIGIN = (4200.0, -1800.0, 35.0)
SEQ_A, SEQ_B = "segment-13572468_oyster", "segment-24681357_oyster"
MAX_PREDICTION_NUM_A, REMOVE_SHORT_TRACK_A = 4, 3
N_FRAMES_B = 120
OUT = os.path.join(HERE, "oyster.npz")

# Run B's timeline: name -> (first frame, last frame, (l, w, h), distance from the path, bearing in degrees, speed per frame)
B_TRACKS = dict(
    first_alone=(0, 15, (4.4, 1.9, 1.6), 14.0, 40.0, 0.10),       # alone in frames 0..9: 6 entries are left
    long=(10, 104, (4.8, 2.0, 1.7), 22.0, 100.0, 0.30),           # 95 entries: top_len 4
    medium=(10, 79, (4.2, 1.8, 1.5), 18.0, 200.0, 0.25),          # 70 entries: int(70 * 0.05...) = 3
    walker=(30, 104, (0.7, 0.6, 1.7), 12.0, 300.0, 0.08),
    rider=(12, 50, (1.8, 0.7, 1.7), 26.0, 150.0, 0.35),
    low=(20, 60, (2.0, 1.2, 0.5), 30.0, 250.0, 0.0),              # Dis_Small in every frame
    tall=(20, 60, (6.0, 2.5, 3.6), 34.0, 340.0, 0.0),             # Dis_Large in every frame
    crossing=(14, 96, (4.6, 1.9, 1.6), 9.0, 20.0, 0.45),
    last_alone=(100, 115, (4.5, 1.9, 1.6), 16.0, 60.0, 0.12))     # alone in frames 105..115: 5 entries are left


def config_a():
    from cpd_amd.oyster import OYSTER_GENERATOR_CONFIG
    g = copy.deepcopy(OYSTER_GENERATOR_CONFIG)
    g["max_prediction_num"], g["remove_short_track"] = MAX_PREDICTION_NUM_A, REMOVE_SHORT_TRACK_A
    return dict(InitLabelGenerator='OYSTER', GeneratorConfig=g)


def config_b():
    from cpd_amd.oyster import OYSTER_CONFIG
    return copy.deepcopy(OYSTER_CONFIG)


def sequence_a(seed=SEED):
    """(frames, poses): odd frames float16, even frames float32."""
    from cpd_amd import synthetic
    frames, poses = synthetic.ppscore_sequence(seed, N_FRAMES_A, N_AZ, np.float32, ORIGIN)
    return [f.astype(np.float16) if k % 2 else f for k, f in enumerate(frames)], poses


def box_drive(seed=SEED, n_frames=N_FRAMES_B):
    """Run B's input: per frame dict(pose, outline_box [k, 7] float64 in the frame's own coordinates). The ego moves 0.35 m and
    yaws 0.2 deg per frame; every object moves at constant velocity along its heading; position, size and heading carry a
    little noise per frame (the tracker's size / yaw windows have something to smooth)."""
    rng = np.random.default_rng(seed + 7000)
    tracks = []
    for first, last, size, dist, bearing, speed in B_TRACKS.values():
        ang = np.deg2rad(bearing)
        start = np.array([0.35 * first + dist * np.cos(ang), dist * np.sin(ang)])
        yaw = rng.uniform(-np.pi, np.pi)
        tracks.append((first, last, size, start, yaw, speed))
    infos = []
    for k in range(n_frames):
        ego_yaw = np.deg2rad(0.2) * k
        ego = np.array([0.35 * k, 0.05 * np.sin(0.3 * k)])
        cs, sn = np.cos(ego_yaw), np.sin(ego_yaw)
        pose = np.eye(4)
        pose[:2, :2] = [[cs, -sn], [sn, cs]]
        pose[:3, 3] = [ego[0] + ORIGIN[0], ego[1] + ORIGIN[1], ORIGIN[2]]
        rows = []
        for first, last, size, start, yaw, speed in tracks:
            noise = rng.uniform(-1, 1, 7)                   # drawn for every track in every frame: a track's rows do not move
            if not first <= k <= last:                      # when another track's span is edited
                continue
            world = start + speed * (k - first) * np.array([np.cos(yaw), np.sin(yaw)]) + 0.05 * noise[0:2]
            rel = world - ego
            l, w, h = size[0] + 0.25 * noise[3], size[1] + 0.12 * noise[4], size[2] + 0.05 * noise[5]
            rows.append([cs * rel[0] + sn * rel[1], -sn * rel[0] + cs * rel[1], h / 2 + 0.02 * noise[2], l, w, h,
                         yaw - ego_yaw + 0.03 * noise[6]])
        infos.append(dict(pose=pose, outline_box=np.array(rows, np.float64).reshape(-1, 7)))
    return infos


def drive_digest(infos):
    h = hashlib.sha256()
    for info in infos:
        h.update(np.ascontiguousarray(info['pose']).tobytes())
        h.update(np.ascontiguousarray(info['outline_box']).tobytes())
    return h.hexdigest()


def write_box_drive(root, infos, seq=SEQ_B):
    os.makedirs(os.path.join(root, seq), exist_ok=True)
    with open(os.path.join(root, seq, seq + "_outline_MFCF.pkl"), "wb") as f:
        pickle.dump([dict(pose=i['pose'].copy(), outline_box=i['outline_box'].copy()) for i in infos], f)


def unpack_infos(z, prefix, n):
    return [dict(outline_box=z["%s%d_box" % (prefix, i)], outline_ids=z["%s%d_ids" % (prefix, i)],
                 outline_cls=z["%s%d_cls" % (prefix, i)], outline_dif=z["%s%d_dif" % (prefix, i)]) for i in range(n)]


def frame_boxes(z, i):
    b = z["pfa%d_box" % i]
    return b.copy() if len(b) else []


def same_infos(got, want, atol=1e-9):
    """None, or the first difference as text."""
    if len(got) != len(want):
        return "%d frames against %d" % (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ('outline_box', 'outline_ids', 'outline_cls', 'outline_dif'):
            if np.asarray(g[k]).shape != np.asarray(w[k]).shape:
                return "frame %d %s: shape %r against %r" % (i, k, np.asarray(g[k]).shape, np.asarray(w[k]).shape)
        if len(w['outline_ids']) == 0:
            continue
        for k in ('outline_ids', 'outline_cls', 'outline_dif'):
            if not np.array_equal(g[k], w[k]):
                return "frame %d %s differs" % (i, k)
        err = np.abs(np.asarray(g['outline_box']) - np.asarray(w['outline_box'])).max()
        if not err <= atol:
            return "frame %d boxes differ by %g" % (i, err)
    return None


def run(seed, verbose=True):
    """The reference over both inputs of `seed`: (arrays to store, counts, failed conditions)."""
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    import ref_oyster as RO
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import cpd.unsupervised_core.ground_removal as gr
    import cpd.unsupervised_core.outline_utils as ou
    import cpd.unsupervised_core.oyster as oy

    rec = {}
    real_ts = ou.TrackSmooth

    class RecordingTrackSmooth(real_ts):
        def tracking(self, all_objects, all_pose, scores=None):
            rec["labels"] = [np.array(b, np.float64).reshape(-1, 7).copy() for b in all_objects]   # before it mutates them
            rec["tracker"] = self
            return super().tracking(all_objects, all_pose, scores)

    def reference(seq, root, cfg):
        unstable_np = gr.np
        gr.np, oy.TrackSmooth = _StableNumpy(), RecordingTrackSmooth
        try:
            infos = oy.OYSTER(seq, root, namespace(cfg))()
        finally:
            gr.np, oy.TrackSmooth = unstable_np, real_ts
        with open(os.path.join(root, seq, seq + "_outline_OYSTER.pkl"), "rb") as f:
            assert len(pickle.load(f)) == len(infos)
        trk = rec.pop("tracker").tracker
        every = list(trk.dead_trajectories.values()) + list(trk.active_trajectories.values())
        short = cfg["GeneratorConfig"]["remove_short_track"]
        met = dict(died=len(trk.dead_trajectories),
                   removed_short=sum(1 for t in every if t.last_updated_timestamp - t.first_updated_timestamp < short))
        return infos, rec.pop("labels"), met

    frames, poses = sequence_a(seed)
    drive = box_drive(seed)
    with tempfile.TemporaryDirectory() as root:
        write_sequence(root, frames, poses, seq=SEQ_A)
        ref_a, labels_a, met_a = reference(SEQ_A, root, config_a())
        write_box_drive(root, drive)
        ref_b, labels_b, met_b = reference(SEQ_B, root, config_b())
    for lab, info in zip(labels_b, drive):
        assert np.array_equal(lab, info['outline_box']), "run B: the tracker's input is not the pickle's boxes"

    out = dict(seed=np.array(seed), n_frames_a=np.array(N_FRAMES_A), n_az=np.array(N_AZ), n_frames_b=np.array(N_FRAMES_B),
               digest_a=np.array(digest(frames, poses)), digest_b=np.array(drive_digest(drive)))
    # run A's per-frame boxes beside the closed-hull restatement (§5l): a flag per box where it leaves the reference by > 1e-9
    import ref_outline as R
    gcfg_a = config_a()["GeneratorConfig"]
    n_flag, count_diff = 0, []
    for i, b in enumerate(labels_a):
        clusters, _ = R.clustering(R.remove_ground(frames[i][:, 0:3], gcfg_a), gcfg_a)
        rb, kept = R.box_fit(clusters, gcfg_a, return_index=True)
        rb = np.asarray(rb, np.float64).reshape(-1, 7)
        if rb.shape != b.shape:       # a hull edge moved a box across a size filter: another seed
            count_diff.append("run A frame %d: %d boxes, the reference has %d" % (i, len(rb), len(b)))
            rb = b + 1.0
        flag = (np.abs(rb - b).max(1) > 1e-9) if len(b) else np.zeros(0, bool)
        if len(kept) == len(b):       # and make_golden_outline's flags: the open hull, Qhull's vertex set, tied best scores
            flag = flag | np.array([cluster_flags(clusters[k], R) != 0 for k in kept], bool)
        out["pfa%d_box" % i], out["pfa%d_flag" % i] = b, flag
        n_flag += int(flag.sum())
    for prefix, infos in (("fina", ref_a), ("finb", ref_b)):
        for i, info in enumerate(infos):
            out["%s%d_box" % (prefix, i)], out["%s%d_ids" % (prefix, i)] = np.asarray(info['outline_box']), np.asarray(info['outline_ids'])
            out["%s%d_cls" % (prefix, i)], out["%s%d_dif" % (prefix, i)] = np.asarray(info['outline_cls']), np.asarray(info['outline_dif'])

    failed, counts = count_diff, dict(flagged_a=n_flag, died_a=met_a["died"], removed_short_a=met_a["removed_short"],
                                      died_b=met_b["died"], removed_short_b=met_b["removed_short"])
    for k in ("died_a", "removed_short_a"):
        if counts[k] < 1:
            failed.append("run A: no track %s" % k)
    stats = {}
    for name, labels, ps, cfg, ref in (("a", labels_a, poses, config_a(), ref_a),
                                       ("b", labels_b, [i['pose'] for i in drive], config_b(), ref_b)):
        st = {}
        got = RO.generate(labels, ps, cfg["GeneratorConfig"], st)
        diff = same_infos(got, ref)
        if diff:
            failed.append("run %s: the restatement leaves the reference: %s" % (name.upper(), diff))
        stats[name] = st
        counts["boxes_in_" + name] = sum(len(b) for b in labels)
        counts["boxes_out_" + name] = sum(len(i['outline_box']) for i in ref)
        counts["tracks_" + name] = len(st["lengths"])
        counts["kept_tracks_" + name] = sum(1 for n in st["lengths"] if n >= 6)
        for k in ("lone_frames", "empty_frames", "dropped_small", "dropped_large", "tied_dis"):
            counts["%s_%s" % (k, name)] = int(st[k])
        for k in range(4):
            counts["corner%d_%s" % (k, name)] = st["corner"][k]
    lengths = stats["a"]["lengths"] + stats["b"]["lengths"]
    counts["len5"], counts["len6"] = lengths.count(5), lengths.count(6)
    counts["len_ge80"], counts["len_60_79"] = sum(1 for n in lengths if n >= 80), sum(1 for n in lengths if 60 <= n < 80)
    for k in ("len5", "len6", "len_ge80", "len_60_79"):
        if counts[k] < 1:
            failed.append("no track with %s" % k)
    for k in ("lone_frames", "empty_frames", "dropped_small", "dropped_large"):
        if counts[k + "_a"] + counts[k + "_b"] < 1:
            failed.append("no %s" % k)
    for k in range(4):
        if counts["corner%d_a" % k] + counts["corner%d_b" % k] < 1:
            failed.append("candidate corner %d never chosen" % k)
    if counts["tied_dis_a"] + counts["tied_dis_b"]:
        failed.append("equal distances within a track")
    if n_flag > 0.10 * sum(len(b) for b in labels_a):
        failed.append("%d of run A's per-frame boxes flagged" % n_flag)
    if counts["kept_tracks_a"] < 3:
        failed.append("run A keeps fewer than 3 tracks")
    out["counts_keys"] = np.array(sorted(counts))
    out["counts_vals"] = np.array([counts[k] for k in out["counts_keys"]], np.int64)
    out["lengths_a"], out["lengths_b"] = np.array(stats["a"]["lengths"], np.int64), np.array(stats["b"]["lengths"], np.int64)
    if verbose:
        print("seed %d: %r" % (seed, counts))
        print("   track lengths A %r B %r" % (stats["a"]["lengths"], stats["b"]["lengths"]))
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
