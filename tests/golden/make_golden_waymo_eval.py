#!/usr/bin/env python3
"""Golden vectors of the Waymo-protocol detection metrics (tests/golden/waymo_eval.npz). Only DATA is written.

The metric op lives in a library outside the reference tree, so nothing here is "the reference's output" except the
IoU cross-check; the rest is closed forms and the independent restatement (tests/ref_waymo_eval.py):
  * ana_a / ana_b [n, 7] float32 and ana_iou [n]: box pairs with closed-form IoU (equal axis-aligned boxes shifted by d
    along x or y: (L - d) / (L + d); identical, touching, contained boxes; a 90 degree rotation; a unit square at 45
    degrees against an axis-aligned one; z-only overlap; headings equal modulo 2 pi);
  * ref_a / ref_b [m, 7] float32 and ref_iou [m]: IoUs of random pairs by the reference's own box3d_iou
    (cpd/unsupervised_core/rotate_iou_cpu_eval.py:85-120, imported by file path; build container only), fed corners built
    in float64 from the float32 boxes in its convention (corner rows 0..3 the top face, 4..7 the bottom face, (x, z) the
    BEV plane with rows 3, 2, 1, 0 counter-clockwise, y up) -- that mapping is exact, no rounding is added. Pairs whose
    intersection polygon its ConvexHull rejects (degenerate) are left out;
  * a seeded 40-frame scene set as Dataset.evaluation's infos (pd_* / gt_* flat arrays) with the restatement's counts,
    heading sums and result dict (counts, ha, keys, values), and a 6-frame set whose raw scores exceed 1 (lg_*).
The scene seed is advanced until the set meets the input conditions the tests rely on (asserted below): no IoU within
1e-4 of its type's threshold; every problem's optimal matching at every cut-off unchanged under five random +-1e-7
perturbations of the weights; greedy-by-score differing from the optimum in at least a tenth of the problems with two or
more edges; at least one problem re-routing an earlier match when a lower-scored row arrives; and the coverage cases
(scores equal to a cut-off, a frame without predictions, one without ground truths, a type without ground truths, level-2
ground truths that absorb predictions).
Usage:  python tests/golden/make_golden_waymo_eval.py
"""
import importlib.util
import os
import sys

import numpy as np

REF = os.environ.get("CPD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import ref_waymo_eval as R  # noqa: E402

CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Truck', 'Cyclist']
SIZES = {'Vehicle': (4.6, 2.0, 1.6), 'Pedestrian': (0.8, 0.7, 1.7), 'Truck': (8.0, 2.6, 3.0), 'Cyclist': (1.8, 0.7, 1.7)}


# ---- analytic IoU cases ---------------------------------------------------------------------------------------------

def analytic_cases():
    a, b, v = [], [], []

    def add(x, y, iou):
        a.append(x), b.append(y), v.append(iou)
    L, W, H = 4.0, 2.0, 1.5
    for d in (0.5, 1.0, 2.5):
        add([0, 0, 0, L, W, H, 0], [d, 0, 0, L, W, H, 0], (L - d) / (L + d))
        add([1, -2, 0.5, L, W, H, 0], [1, -2 + d * 0.5, 0.5, L, W, H, 0], (W - d * 0.5) / (W + d * 0.5))
    add([3, 4, 1, L, W, H, 0.7], [3, 4, 1, L, W, H, 0.7], 1.0)                       # identical
    add([0, 0, 0, L, W, H, 0], [L, 0, 0, L, W, H, 0], 0.0)                           # touching along x
    add([0, 0, 0, L, W, H, 0], [0, 0, H, L, W, H, 0], 0.0)                           # touching along z
    add([2, 1, 0, 1.0, 0.5, 0.5, 0.3], [2, 1, 0, L, W, H, 0.3], 0.25 / (L * W * H))  # contained
    add([0, 0, 0, L, W, H, 0], [0, 0, 0, L, W, H, np.float32(np.pi / 2)], 1.0 / 3.0)  # 90 degrees: a 2 x 2 square
    oct_area = 2.0 * (np.sqrt(2.0) - 1.0)                                            # unit square at 45 degrees
    add([0, 0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, np.float32(np.pi / 4)], oct_area / (2.0 - oct_area))
    add([0, 0, 0, L, W, 2.0, 0.25], [0, 0, 1.0, L, W, 2.0, 0.25], 1.0 / 3.0)         # z-only: half the height overlaps
    add([0, 0, 0, L, W, 2.0, 0.25], [0, 0, 3.0, L, W, 2.0, 0.25], 0.0)               # z intervals apart
    # headings equal modulo 2 pi: a float32 heading whose float32(heading + 2 pi) is off by < 5e-9 rad (the IoU moves by about that much)
    cand = np.linspace(0.01, 0.12, 200001).astype(np.float32)
    err = np.abs((cand.astype(np.float64) + 2 * np.pi).astype(np.float32).astype(np.float64) - (cand.astype(np.float64) + 2 * np.pi))
    th = cand[int(np.argmin(err))]
    assert err.min() < 5e-9
    add([5, -3, 0, L, W, H, th], [5, -3, 0, L, W, H, np.float32(np.float64(th) + 2 * np.pi)], 1.0)
    return np.array(a, np.float32), np.array(b, np.float32), np.array(v, np.float64)


# ---- the reference's box3d_iou --------------------------------------------------------------------------------------

def load_reference_iou():
    path = os.path.join(REF, "cpd", "unsupervised_core", "rotate_iou_cpu_eval.py")
    spec = importlib.util.spec_from_file_location("ref_rotate_iou_cpu_eval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.box3d_iou


def reference_corners(box):
    box = np.asarray(box, np.float32).astype(np.float64)
    ccw = R.corners_bev(box)
    out = np.zeros((8, 3))
    for i in range(4):
        x, y = ccw[3 - i]
        out[i] = (x, box[2] + box[5] / 2, y)
        out[i + 4] = (x, box[2] - box[5] / 2, y)
    return out


def reference_pairs(rng, n=200):
    box3d_iou = load_reference_iou()
    a, b, v = [], [], []
    while len(a) < n:
        ba = np.array([*rng.uniform(-60, 60, 2), rng.uniform(-1, 2), rng.uniform(0.5, 8), rng.uniform(0.4, 3),
                       rng.uniform(0.5, 3), rng.uniform(-np.pi, np.pi)], np.float32)
        if len(a) % 4 == 3:       # an unrelated box nearby
            bb = np.array([*(ba[:2] + rng.uniform(-4, 4, 2)), rng.uniform(-1, 2), rng.uniform(0.5, 8), rng.uniform(0.4, 3),
                           rng.uniform(0.5, 3), rng.uniform(-np.pi, np.pi)], np.float32)
        else:                     # a jittered copy
            bb = (ba + np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 0.2, 3), [rng.normal(0, 0.3)]])).astype(np.float32)
            bb[3:6] = np.maximum(bb[3:6], 0.3)
        try:
            iou, _ = box3d_iou(reference_corners(ba), reference_corners(bb))
        except Exception:         # its ConvexHull rejects a degenerate intersection polygon
            continue
        if not np.isfinite(iou):
            continue
        a.append(ba), b.append(bb), v.append(float(iou))
    return np.array(a, np.float32), np.array(b, np.float32), np.array(v, np.float64)


# ---- scenes ---------------------------------------------------------------------------------------------------------

def to_fake_lidar(centre_boxes):
    """Inverse of the estimator's fake-lidar conversion: (x, y, z centre, dx, dy, dz, heading) -> (x, y, z bottom, w, l, h, r)."""
    b = np.asarray(centre_boxes, np.float64).reshape(-1, 7)
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 5] / 2, b[:, 4], b[:, 3], b[:, 5], -b[:, 6] - np.pi / 2], 1)


def shifted(box, along, rng, jitter=0.0):
    """`box` moved by `along` x its length in its heading direction, plus a small jitter."""
    out = np.array(box, np.float64)
    out[0] += np.cos(box[6]) * along * box[3] + rng.normal(0, jitter)
    out[1] += np.sin(box[6]) * along * box[3] + rng.normal(0, jitter)
    return out


def make_scenes(seed, n_frames=40, logits=False):
    rng = np.random.default_rng(seed)
    pd_infos, gt_infos = [], []
    for f in range(n_frames):
        gts, gnames, gdiff, gpts, pds, pnames, pscores = [], [], [], [], [], [], []

        def new_gt(name, far=False):
            l, w, h = np.array(SIZES[name]) * rng.uniform(0.85, 1.15, 3)
            r = rng.uniform(105, 130) if far else rng.uniform(3, 70)
            phi = rng.uniform(-np.pi, np.pi)
            return np.array([r * np.cos(phi), r * np.sin(phi), rng.uniform(-0.5, 1.0), l, w, h, rng.uniform(-np.pi, np.pi)])

        def put_gt(box, name):
            gts.append(box), gnames.append(name)
            pts = int(rng.choice([0, 3, 5, 6, 40, 200], p=[0.06, 0.12, 0.08, 0.1, 0.32, 0.32]))
            gpts.append(pts)
            gdiff.append(int(rng.choice([0, 0, 0, 2])))         # mostly unset (0): decided by the point count

        def put_pd(box, name, score):
            pds.append(box), pnames.append(name), pscores.append(score)

        def new_score():
            s = rng.uniform(0.02, 0.99)
            if rng.uniform() < 0.2:
                s = float(np.float32(int(rng.integers(1, 100)) * 0.01))     # exactly on a cut-off
            return 6.0 * s - 3.0 if logits else s

        if f not in (5,):                                                    # frame 5: no ground truths
            for _ in range(int(rng.integers(3, 11))):
                name = str(rng.choice(['Vehicle', 'Pedestrian', 'Cyclist', 'Sign'], p=[0.5, 0.3, 0.15, 0.05]))
                put_gt(new_gt(name if name != 'Sign' else 'Pedestrian', far=rng.uniform() < 0.05), name)
        n_plain = len(gts)
        if f not in (3,):                                                    # frame 3: no predictions
            for g in range(n_plain):
                if gnames[g] == 'Sign':
                    continue
                name = gnames[g]
                for _ in range(int(rng.choice([0, 1, 1, 1, 2]))):
                    tight = rng.uniform(0.02, 0.12) if name == 'Vehicle' else rng.uniform(0.03, 0.2)
                    box = shifted(gts[g], rng.choice([-1, 1]) * tight, rng, 0.02)
                    box[3:6] *= rng.uniform(0.95, 1.05, 3)
                    box[6] += rng.normal(0, 0.05) + (np.pi if rng.uniform() < 0.1 else 0.0)
                    put_pd(box, name if rng.uniform() > 0.05 else 'Truck', new_score())
            for _ in range(int(rng.integers(0, 5))):                         # unrelated boxes
                name = str(rng.choice(CLASS_NAMES))
                put_pd(new_gt(name, far=rng.uniform() < 0.1), name, new_score())
            # conflict clusters: two (or three) ground truths a fraction of a length apart; the best-scored prediction
            # sits between the first two, a little nearer the first, and a lower-scored one reaches only the first
            for _ in range(0 if f == 5 else int(rng.choice([0, 1, 1, 2]))):
                name = str(rng.choice(['Vehicle', 'Pedestrian', 'Cyclist']))
                k = 0.13 / 0.3 if name == 'Vehicle' else 1.0                 # shifts scaled to the type's threshold
                a = new_gt(name)
                chain = [a, shifted(a, 0.30 * k, rng)]
                if rng.uniform() < 0.4:
                    chain.append(shifted(a, 0.60 * k, rng))
                for c in chain:
                    put_gt(c, name)
                s = sorted(rng.uniform(0.1, 0.95, len(chain)))[::-1]
                for i in range(len(chain) - 1):
                    put_pd(shifted(a, (0.30 * i + 0.14) * k, rng), name, 6.0 * s[i] - 3.0 if logits else s[i])
                put_pd(shifted(a, -0.28 * k, rng), name, 6.0 * s[-1] - 3.0 if logits else s[-1])
        gt_infos.append({"name": np.array(gnames, dtype="<U16"), "difficulty": np.array(gdiff, np.int32),
                         "num_points_in_gt": np.array(gpts, np.int64),
                         "gt_boxes_lidar": to_fake_lidar(np.array(gts).reshape(-1, 7)).astype(np.float32)})
        pd_infos.append({"name": np.array(pnames, dtype="<U16"), "score": np.array(pscores, np.float32),
                         "boxes_lidar": np.array(pds, np.float64).reshape(-1, 7).astype(np.float32)})
    return pd_infos, gt_infos


def matchings(w, score):
    """[(cut-off, frozenset of (row, col))] for every cut-off whose subset differs from the previous one."""
    out, prev = [], None
    for k in range(101):
        idx = np.nonzero(score >= R.CUTOFFS[k])[0]
        if prev is not None and len(idx) == prev:
            continue
        prev = len(idx)
        out.append((k, frozenset((int(idx[r]), c) for r, c in R.optimal_pairs(w[idx]))))
    return out


def conditions(pd_infos, gt_infos, rng, need_cutoff):
    """None when the set meets every input condition, else the reason."""
    flat = R.infos_to_flat(pd_infos, gt_infos)
    a_pd, a_gt = R.infos_from_flat(flat)
    pf, pb, pt, ps, pn, _ = R.generate_waymo_type_results(a_pd, CLASS_NAMES, False)
    gf, gb, gt, gs, _, gd = R.generate_waymo_type_results(a_gt, CLASS_NAMES, True, True)
    pb, pf, pt, ps, pn = R.mask_by_distance(100, pb, pf, pt, ps, pn)
    gb, gf, gt, gs, gd = R.mask_by_distance(100, gb, gf, gt, gs, gd)
    if ps.max() > 1:
        ps = 1 / (1 + np.exp(-ps))
    counts, ha, blocks = R.evaluate_arrays(pf, pb, pt, ps, gf, gb, gt, gd, len(gt_infos))
    ps32 = np.asarray(ps, np.float32)
    multi, differ, reroute, absorbed, on_cutoff = 0, 0, 0, 0, False
    for f, t, order, gi, iou in blocks:
        thr = R.IOU_THRESHOLDS[t]
        if iou.size and np.abs(iou - thr).min() < 1e-4:
            return "an IoU within 1e-4 of %.1f" % thr
        w = np.where(iou >= thr, iou, 0.0)
        score = ps32[order]
        on_cutoff |= bool(np.isin(score, R.CUTOFFS).any())
        base = matchings(w, score)
        for _ in range(5):
            wp = np.where(w > 0, w + rng.uniform(-1e-7, 1e-7, w.shape), 0.0)
            if matchings(wp, score) != base:
                return "a matching that a 1e-7 perturbation changes"
        for (_, hi), (_, lo) in zip(base[1:], base[:-1]):      # base runs from the largest subset (k = 0) down
            held = dict(hi)
            if any(r in held and held[r] != c for r, c in lo):
                reroute += 1
                break
        if np.count_nonzero(w) >= 2:
            multi += 1
            g = R.problem_counts(iou, score, gd[gi], pb[order, 6], gb[gi, 6], thr, R.greedy_pairs)[0]
            o = R.problem_counts(iou, score, gd[gi], pb[order, 6], gb[gi, 6], thr)[0]
            differ += int(not np.array_equal(g, o))
        final = dict((c, r) for r, c in base[0][1]) if base else {}
        absorbed += sum(1 for c in final if gd[gi][c] == 2)
    if differ * 10 < multi:
        return "greedy differs in %d of %d problems" % (differ, multi)
    if reroute < 1:
        return "no re-routed match"
    if need_cutoff and not on_cutoff:
        return "no score on a cut-off"
    if absorbed < 1:
        return "no level-2 ground truth absorbs a prediction"
    if (gt == 3).any() or not (pt == 3).any():
        return "type 3 must have predictions and no ground truth"
    n_pd = np.bincount(pf, minlength=len(gt_infos))
    n_gt = np.bincount(gf, minlength=len(gt_infos))
    if not ((n_pd == 0) & (n_gt > 0)).any() or not ((n_gt == 0) & (n_pd > 0)).any():
        return "needs a frame without predictions and one without ground truths"
    return None, counts, ha, dict(multi=multi, differ=differ, reroute=reroute, absorbed=absorbed)


def checked_scenes(seed, n_frames, logits):
    rng = np.random.default_rng(seed + 1000)
    for s in range(seed, seed + 200):
        pd_infos, gt_infos = make_scenes(s, n_frames, logits)
        res = conditions(pd_infos, gt_infos, rng, not logits)
        if isinstance(res, tuple):
            print("seed %d: %s" % (s, res[3]))
            return pd_infos, gt_infos, res[1], res[2]
        print("seed %d rejected: %s" % (s, res))
    raise RuntimeError("no seed meets the conditions")


def main():
    out = {}
    out["ana_a"], out["ana_b"], out["ana_iou"] = analytic_cases()
    for x, y, v in zip(out["ana_a"], out["ana_b"], out["ana_iou"]):
        assert abs(R.iou_pair(x, y) - v) < 1e-7, (x, y, v, R.iou_pair(x, y))
    out["ref_a"], out["ref_b"], out["ref_iou"] = reference_pairs(np.random.default_rng(20261019))
    worst = max(abs(R.iou_pair(x, y) - v) for x, y, v in zip(out["ref_a"], out["ref_b"], out["ref_iou"]))
    print("restatement vs the reference's box3d_iou: max |diff| = %.3g over %d pairs" % (worst, len(out["ref_iou"])))
    assert worst < 1e-7

    pd_infos, gt_infos, counts, ha = checked_scenes(7, 40, False)
    out.update(R.infos_to_flat(pd_infos, gt_infos))
    result, c2, h2 = R.waymo_evaluation(*R.infos_from_flat(out), CLASS_NAMES)
    assert np.array_equal(c2, counts) and np.array_equal(h2, ha)
    out["counts"], out["ha"] = counts, ha
    out["keys"] = np.array(list(result.keys()))
    out["values"] = np.array([v[0] for v in result.values()], np.float64)

    pd_infos, gt_infos, counts, ha = checked_scenes(107, 6, True)
    assert max(float(i["score"].max()) for i in pd_infos if len(i["score"])) > 1
    out.update(R.infos_to_flat(pd_infos, gt_infos, "lg_"))
    result, _, _ = R.waymo_evaluation(*R.infos_from_flat(out, "lg_"), CLASS_NAMES)
    out["lg_counts"], out["lg_ha"] = counts, ha
    out["lg_values"] = np.array([v[0] for v in result.values()], np.float64)
    out["class_names"] = np.array(CLASS_NAMES)

    path = os.path.join(HERE, "waymo_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    for k, v in zip(out["keys"], out["values"]):
        print("%s: %.4f" % (k, v))


if __name__ == "__main__":
    main()
