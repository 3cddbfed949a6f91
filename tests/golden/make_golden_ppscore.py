#!/usr/bin/env python3
"""Golden vectors of the PP-score precompute, computed by the REFERENCE itself (build container only).

cpd/unsupervised_core/precompute_ppscore.py is run from the reference tree by path (numpy 2 removed np.mat: it is aliased to
np.asmatrix first). Inputs are two cpd_amd.synthetic.ppscore_sequence drives of 14 frames, regenerated from their seeds by the
tests (a digest of every sequence is stored, so a different numpy RNG fails with a clear message):
  A  origin (0, 0, 0);   B  origin (5000, 2500, 0) m, where the float32 rounding in world coordinates is about half a millimetre.
Each is written to a temporary directory as the dataset stores a sequence (float16 NNNN.npy frames, <seq>.pkl with the poses)
and the reference's save_pp_score runs over it twice: max_win 6 / win_inte 1 (frames 6 and 7 see T = 12, the ends T = 6..11)
and the defaults 30 / 5 (T <= 3). Recorded per (sequence, run), frames concatenated: the counts the reference handed to
compute_ephe_score (per frame as [T, N], in the narrowest unsigned type that holds them), the float16 H it saved, the traversal count per frame and the mask of points whose float64 H lies within
1e-9 of a float16 rounding tie (a device log a few ulps from numpy's moves H by less than 1e-14, so only those may differ).
Asserted here: the restatement (tests/ref_ppscore.py) gives the reference's transformed coordinates and counts bit for bit
and its float16 H on every point; in each T = 12 frame between 5 % and 95 % of the points pass H > 0.7; the tie share is
below 1e-3.
Usage:  python tests/golden/make_golden_ppscore.py
"""
import hashlib
import importlib.util
import os
import pickle
import sys
import tempfile

import numpy as np

REF = os.environ.get("CPD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SEQS = {"A": dict(seed=21, origin=(0.0, 0.0, 0.0)), "B": dict(seed=22, origin=(5000.0, 2500.0, 0.0))}
N_FRAMES, N_AZ = 14, 120
RUNS = {"w6": (6, 1), "def": (30, 5)}


def digest(frames, poses):
    h = hashlib.sha256()
    for f, p in zip(frames, poses):
        h.update(np.ascontiguousarray(f).tobytes())
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def load_reference():
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    spec = importlib.util.spec_from_file_location(
        "ref_precompute_ppscore", os.path.join(REF, "cpd", "unsupervised_core", "precompute_ppscore.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_sequence(root, seq, frames, poses):
    os.makedirs(os.path.join(root, seq))
    for i, f in enumerate(frames):
        np.save(os.path.join(root, seq, "%04d.npy" % i), f)
    with open(os.path.join(root, seq, seq + ".pkl"), "wb") as f:
        pickle.dump([{"pose": p} for p in poses], f)


def main():
    from cpd_amd import synthetic
    import ref_ppscore as R
    ref = load_reference()
    seen = {}
    ephe, ppscore = ref.compute_ephe_score, ref.compute_ppscore

    def rec_ephe(count):
        H = ephe(count)
        seen["count"], seen["H"] = np.array(count), np.array(H)
        return H

    def rec_ppscore(cur_frame, neighbor_traversals=None, max_neighbor_dist=0.3):
        seen["trav"] = [np.array(t) for t in neighbor_traversals]
        return ppscore(cur_frame, neighbor_traversals, max_neighbor_dist)

    ref.compute_ephe_score, ref.compute_ppscore = rec_ephe, rec_ppscore
    out = dict(n_frames=np.array(N_FRAMES), n_az=np.array(N_AZ), seqs=np.array(sorted(SEQS)),
               runs=np.array(sorted(RUNS)), run_args=np.array([RUNS[k] for k in sorted(RUNS)]))
    for name, s in SEQS.items():
        frames, poses = synthetic.ppscore_sequence(s["seed"], N_FRAMES, N_AZ, np.float16, s["origin"])
        out[name + "_seed"], out[name + "_origin"] = np.array(s["seed"]), np.array(s["origin"])
        out[name + "_digest"] = np.array(digest(frames, poses))
        out[name + "_n"] = np.array([len(f) for f in frames], np.int32)
        for run, (max_win, win_inte) in RUNS.items():
            counts, hs, ties, ts, unfused = [], [], [], [], [0, 0]
            with tempfile.TemporaryDirectory() as root:
                seq = "segment-" + name
                write_sequence(root, seq, frames, poses)
                # the reference saves frame i right after computing it: np.save is the hook that checks and records frame i
                saved = np.save

                def save_hook(path, arr, _saved=saved):
                    i = int(os.path.basename(path)[:4])
                    trav = R.frame_traversals(frames, poses, i, max_win, win_inte)
                    assert len(trav) == len(seen["trav"])
                    for a, b in zip(trav, seen["trav"]):
                        assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b), \
                            "restatement: transformed coordinates differ from the reference (frame %d)" % i
                    inv = np.linalg.inv(poses[i])
                    for j, b in zip(R.window(i, N_FRAMES, max_win, win_inte), seen["trav"]):
                        unfused[0] += int((R.rigid_unfused(R.rigid_unfused(frames[j], poses[j]), inv) != b).sum())
                        unfused[1] += b.size
                    c = R.count_neighbors(frames[i][:, 0:3], trav, 0.3)
                    assert np.array_equal(c, seen["count"]), "restatement: counts differ from scipy's (frame %d)" % i
                    H = R.ephe_score(c)
                    assert np.array_equal(H.astype(np.float16), np.asarray(arr)), \
                        "restatement: float16 H differs from the reference (frame %d)" % i
                    assert np.abs(H - seen["H"]).max() <= 1e-12
                    counts.append(seen["count"])
                    hs.append(np.asarray(arr))
                    ties.append(R.tie_mask(seen["H"]))
                    ts.append(c.shape[1])
                    _saved(path, arr)

                ref.np.save = save_hook
                try:
                    assert ref.save_pp_score(seq, root, max_win, win_inte) is True
                finally:
                    ref.np.save = saved
                assert len(hs) == N_FRAMES
            cmax = max(int(c.max()) for c in counts)
            flat = np.concatenate([c.T.reshape(-1) for c in counts])    # per frame [T, N]: columns compress better
            p = "%s_%s_" % (name, run)
            out[p + "counts"] = flat.astype(np.uint8 if cmax < 256 else np.uint16 if cmax < 65536 else np.int32)
            out[p + "h"] = np.concatenate(hs).astype(np.float16)
            tie = np.concatenate(ties)
            out[p + "tie"] = np.packbits(tie)
            out[p + "T"] = np.array(ts, np.int32)
            share = tie.mean()
            assert share < 1e-3, "tie share %g" % share
            pass_share = [float((h.astype(np.float64) > 0.7).mean()) for h in hs]
            for i, t in enumerate(ts):
                if t == 12:
                    assert 0.05 < pass_share[i] < 0.95, "frame %d: %.3f of the points pass H > 0.7" % (i, pass_share[i])
            print("%s %s: T per frame %s, max count %d, tie points %d of %d, share of H > 0.7 per frame %s" % (
                name, run, ts, cmax, int(tie.sum()), len(tie), np.round(pass_share, 3).tolist()))
            print("    unfused (m0 x + m1 y) + m2 z + m3 products: %d of %d transformed coordinates differ from the reference" %
                  tuple(unfused))
        assert 12 in out[name + "_w6_T"]
    path = os.path.join(HERE, "ppscore.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
