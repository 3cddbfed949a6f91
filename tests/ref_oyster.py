"""Numpy restatement of what is OYSTER's own in cpd/unsupervised_core/oyster.py: the half of generate_outline_box that follows
the tracker (l.70-148) and outline_utils.py corner_align (l.94-123). Written from the behaviour list of DESIGN §5q, one track
at a time; the tracker is cpd_amd.tracker (checked against the reference in test_mfcf_ref.py).

Behaviours kept: a frame counts only when more than one object survives drop_cls; tracks are kept per id in first-seen order;
fewer than six entries: neither aligned nor written; the size consensus is the mean l, w over the top_len(n) boxes nearest the
origin, added in rank order; corner_align takes the candidate of the GREATEST norm, the first on ties, through a float32 pose;
rows of a frame follow the first appearance of their track; empty frames get (0, 7) and (0,) float arrays.
"""
import numpy as np

MIN_TRACK_LEN = 6
DROPPED = ('Dis_Small', 'Dis_Large')
SIGNS = ((1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0))      # the candidates, in the order they are tried


def top_len(n):
    return max(3, int(n * (1 - 0.95)))


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def candidates(boxes, l_off, w_off):
    """The four candidate centres of every box: (x' [4, n], y' [4, n], z' [n], norm [4, n])."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    c, s = _f32(np.cos(boxes[:, 6])), _f32(np.sin(boxes[:, 6]))
    tx, ty, tz = _f32(boxes[:, 0]), _f32(boxes[:, 1]), _f32(boxes[:, 2])
    hx, hy = np.asarray(l_off, np.float64) / 2, np.asarray(w_off, np.float64) / 2
    px = np.stack([((sx * hx) * c + (sy * hy) * (-s)) + tx for sx, sy in SIGNS])
    py = np.stack([((sx * hx) * s + (sy * hy) * c) + ty for sx, sy in SIGNS])
    norm = np.sqrt(((px * px + py * py) + tz * tz) + 1.0)
    return px, py, tz, norm


def corner_align(box, l_off, w_off, return_choice=False):
    """One box [7] -> a new box: l += l_off, w += w_off, the centre moved to the chosen candidate, z = float32(z)."""
    px, py, tz, norm = candidates(np.asarray(box, np.float64)[None], [l_off], [w_off])
    k = int(np.argmax(norm[:, 0]))                 # the first of the greatest
    out = np.array(box, np.float64)
    out[0], out[1], out[2] = px[k, 0], py[k, 0], tz[0]
    out[3] += l_off
    out[4] += w_off
    return (out, k) if return_choice else out


def consensus(boxes):
    """(mean_l, mean_w) of a track's boxes [n, 7]: over the top_len(n) rows nearest the origin, added in rank order."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    x, y, z = boxes[:, 0], boxes[:, 1], boxes[:, 2]
    order = np.argsort(np.sqrt((x * x + y * y) + z * z), kind="stable")
    near = order[:top_len(len(boxes))]
    sum_l = sum_w = 0.0
    for r in near:
        sum_l, sum_w = sum_l + boxes[r, 3], sum_w + boxes[r, 4]
    return sum_l / len(near), sum_w / len(near)


def align_track(boxes, return_choice=False):
    """A track's boxes [n, 7] in frame order -> the aligned boxes [n, 7] (and the candidate taken per box)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    mean_l, mean_w = consensus(boxes)
    l_off, w_off = mean_l - boxes[:, 3], mean_w - boxes[:, 4]
    px, py, tz, norm = candidates(boxes, l_off, w_off)
    k = np.argmax(norm, axis=0)
    rows = np.arange(len(boxes))
    out = boxes.copy()
    out[:, 0], out[:, 1], out[:, 2] = px[k, rows], py[k, rows], tz
    out[:, 3] = boxes[:, 3] + l_off
    out[:, 4] = boxes[:, 4] + w_off
    return (out, k) if return_choice else out


def align_tracks(boxes, track_off):
    """Track-major boxes [N, 7] with offsets [T + 1] -> aligned [N, 7]: what cpd_oyster_align_tracks computes."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    out = np.empty_like(boxes)
    for a, b in zip(track_off[:-1], track_off[1:]):
        if b > a:
            out[a:b] = align_track(boxes[a:b])
    return out


def tie_tracks():
    """Hand-built tracks in which candidates coincide: every l equal (l_off == 0: candidates 0 and 3, 1 and 2 are the same
    point), every w equal (0 and 2, 1 and 3), both (all four). Sizes are exact in binary, so the means are the sizes
    themselves. Returns (boxes [N, 7] track-major, track_off, the candidates that may win per track)."""
    rng = np.random.default_rng(21)
    tracks, allowed = [], []
    for same_l, same_w in ((True, False), (False, True), (True, True)):
        n = 9
        ang = rng.uniform(-np.pi, np.pi, n)
        r = rng.uniform(5, 40, n)
        b = np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(0.5, 1.2, n),
                      np.full(n, 4.5) if same_l else rng.uniform(3.5, 5.5, n),
                      np.full(n, 2.0) if same_w else rng.uniform(1.5, 2.5, n),
                      rng.uniform(1.4, 1.9, n), rng.uniform(-np.pi, np.pi, n)], 1)
        tracks.append(b)
        allowed.append((0,) if same_l and same_w else (0, 1))
    off = np.zeros(len(tracks) + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in tracks])
    return np.concatenate(tracks), off, allowed


def surviving(objs, ids, cls, dif):
    keep = np.ones(len(ids), bool)
    for name in DROPPED:
        keep &= np.asarray(cls) != name
    return objs[keep], ids[keep], cls[keep], dif[keep]


def after_tracker(per_frame, stats=None):
    """per_frame[i] = (objs [k, 7], ids, cls names, dif) as TrackSmooth.get_current_frame_objects_and_cls(i) returns them.
    Returns per frame a dict of outline_box / outline_ids / outline_cls / outline_dif. stats (a dict) receives the counts the
    golden generator asserts on."""
    tracks = {}
    st = dict(lone_frames=0, empty_frames=0, dropped_small=0, dropped_large=0, corner=[0, 0, 0, 0], lengths=[], tied_dis=0)
    for i, (objs, ids, cls, dif) in enumerate(per_frame):
        st["dropped_small"] += int((np.asarray(cls) == 'Dis_Small').sum()) if len(ids) else 0
        st["dropped_large"] += int((np.asarray(cls) == 'Dis_Large').sum()) if len(ids) else 0
        if len(ids):
            objs, ids, cls, dif = surviving(objs, ids, cls, dif)
        st["lone_frames"] += len(ids) == 1
        st["empty_frames"] += len(ids) == 0
        if len(ids) <= 1:
            continue
        for j, ob_id in enumerate(ids):
            tracks.setdefault(ob_id, []).append((i, objs[j], cls[j], dif[j]))
    frames = {}
    for ob_id, entries in tracks.items():
        st["lengths"].append(len(entries))
        if len(entries) < MIN_TRACK_LEN:
            continue
        boxes = np.array([e[1] for e in entries])
        dis = np.sqrt((boxes[:, 0] * boxes[:, 0] + boxes[:, 1] * boxes[:, 1]) + boxes[:, 2] * boxes[:, 2])
        st["tied_dis"] += len(dis) - len(np.unique(dis))
        aligned, choice = align_track(boxes, return_choice=True)
        for k in choice:
            st["corner"][k] += 1
        for (i, _, cls, dif), box in zip(entries, aligned):
            frames.setdefault(i, []).append((box, ob_id, cls, dif))
    out = []
    for i in range(len(per_frame)):
        if i in frames:
            out.append(dict(outline_box=np.array([r[0] for r in frames[i]]), outline_ids=np.array([r[1] for r in frames[i]]),
                            outline_cls=np.array([r[2] for r in frames[i]]), outline_dif=np.array([r[3] for r in frames[i]])))
        else:
            out.append(dict(outline_box=np.empty((0, 7)), outline_ids=np.empty((0,)), outline_cls=np.empty((0,)),
                            outline_dif=np.empty((0,))))
    if stats is not None:
        stats.update(st)
    return out


def generate(all_labels, all_pose, generator_cfg, stats=None):
    """generate_outline_box from the per-frame boxes on: tracker, collection, alignment, regrouping."""
    from cpd_amd.tracker import TrackSmooth
    ts = TrackSmooth(generator_cfg)
    ts.tracking([np.array(b, np.float64).reshape(-1, 7).copy() if len(b) else [] for b in all_labels],
                [np.array(p, np.float64) for p in all_pose])
    return after_tracker([ts.get_current_frame_objects_and_cls(i) for i in range(len(all_labels))], stats)
