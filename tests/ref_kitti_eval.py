"""Plain-numpy restatement of the KITTI-protocol evaluation (kitti_object_eval_python/eval.py + rotate_iou.py), no numba.

It restates the parts cpd_amd.kitti_eval moves to the GPU -- the overlaps and both matching passes -- vectorised over
pairs / frames / thresholds, with the kernels' arithmetic (float32 polygon clipping, float64 triangle-fan area, float64
criterion arithmetic rounded to float32; numba's sequential sums). The host half (clean_data flags, get_thresholds, the
precision / recall / AOS arithmetic and the result string) is cpd_amd.kitti_eval's own numpy code, run with these stages
in place of the device ones (`get_official_eval_result` below). The golden test checks the whole against the reference's
recorded output; GPU tests check the kernels against this at sizes the reference cannot run in a test.
"""
import contextlib

import numpy as np

N_SAMPLE_PTS = 41
MIN_OVERLAPS = (0.25, 0.5, 0.7)


# ---- rotate_iou.py ----------------------------------------------------------------------------------------------------

def _corners(b):
    """rbbox_to_corners for float32 boxes [P, 5] -> [P, 4, 2] float32."""
    a_cos, a_sin = np.cos(b[:, 4]), np.sin(b[:, 4])
    hx, hy = -b[:, 2] / np.float32(2), -b[:, 3] / np.float32(2)
    cx = np.stack([hx, hx, -hx, -hx], 1)
    cy = np.stack([hy, -hy, -hy, hy], 1)
    x = a_cos[:, None] * cx + a_sin[:, None] * cy + b[:, 0:1]
    y = -a_sin[:, None] * cx + a_cos[:, None] * cy + b[:, 1:2]
    return np.stack([x, y], 2).astype(np.float32)


def _in_quad(px, py, c):
    ab0, ab1 = c[:, 1, 0] - c[:, 0, 0], c[:, 1, 1] - c[:, 0, 1]
    ad0, ad1 = c[:, 3, 0] - c[:, 0, 0], c[:, 3, 1] - c[:, 0, 1]
    ap0, ap1 = px - c[:, 0, 0], py - c[:, 0, 1]
    abab, abap = ab0 * ab0 + ab1 * ab1, ab0 * ap0 + ab1 * ap1
    adad, adap = ad0 * ad0 + ad1 * ad1, ad0 * ap0 + ad1 * ap1
    return (abab >= abap) & (abap >= 0) & (adad >= adap) & (adap >= 0)


def _segment(p1, p2, i, j):
    A0, A1 = p1[:, i, 0], p1[:, i, 1]
    B0, B1 = p1[:, (i + 1) % 4, 0], p1[:, (i + 1) % 4, 1]
    C0, C1 = p2[:, j, 0], p2[:, j, 1]
    D0, D1 = p2[:, (j + 1) % 4, 0], p2[:, (j + 1) % 4, 1]
    BA0, BA1, DA0, CA0, DA1, CA1 = B0 - A0, B1 - A1, D0 - A0, C0 - A0, D1 - A1, C1 - A1
    acd = DA1 * CA0 > CA1 * DA0
    bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0)
    abc = CA1 * BA0 > BA1 * CA0
    abd = DA1 * BA0 > BA1 * DA0
    DC0, DC1 = D0 - C0, D1 - C1
    ABBA, CDDC = A0 * B1 - B0 * A1, C0 * D1 - D0 * C1
    DH = BA1 * DC0 - BA0 * DC1
    return (acd != bcd) & (abc != abd), (ABBA * DC0 - BA0 * CDDC) / DH, (ABBA * DC1 - BA1 * CDDC) / DH


def rotate_iou_pairs(q, b, criterion):
    """devRotateIoUEval(q[p], b[p], criterion) for float32 boxes [P, 5] -> float32 [P]; at most 8 intersection points."""
    q, b = np.asarray(q, np.float32).reshape(-1, 5), np.asarray(b, np.float32).reshape(-1, 5)
    P = q.shape[0]
    with np.errstate(all="ignore"):
        c1, c2 = _corners(q), _corners(b)
        cand, ok = [], []
        for i in range(4):
            cand.append(c1[:, i]); ok.append(_in_quad(c1[:, i, 0], c1[:, i, 1], c2))
            cand.append(c2[:, i]); ok.append(_in_quad(c2[:, i, 0], c2[:, i, 1], c1))
        for i in range(4):
            for j in range(4):
                hit, x, y = _segment(c1, c2, i, j)
                cand.append(np.stack([x, y], 1)); ok.append(hit)
        cand, ok = np.stack(cand, 1), np.stack(ok, 1)                     # [P, 24, 2], [P, 24]
        rank = np.cumsum(ok, 1) - 1
        keep = ok & (rank < 8)
        n = keep.sum(1)
        pts = np.zeros((P, 8, 2), np.float32)
        pi, ci = np.nonzero(keep)
        pts[pi, rank[pi, ci]] = cand[pi, ci]
        # sort_vertex_in_convex_polygon: float32 centre (sequential sums), pseudo-angle keys, insertion sort
        cx, cy = np.zeros(P, np.float32), np.zeros(P, np.float32)
        for k in range(8):
            cx = np.where(k < n, cx + pts[:, k, 0], cx)
            cy = np.where(k < n, cy + pts[:, k, 1], cy)
        nn = np.maximum(n, 1).astype(np.float64)
        cx, cy = (cx.astype(np.float64) / nn).astype(np.float32), (cy.astype(np.float64) / nn).astype(np.float32)
        v0, v1 = pts[:, :, 0] - cx[:, None], pts[:, :, 1] - cy[:, None]
        d = np.sqrt(v0 * v0 + v1 * v1)
        v0, v1 = v0 / d, v1 / d
        vs = np.where(v1 < 0, (-2.0 - v0.astype(np.float64)).astype(np.float32), v0)
        rows = np.arange(P)
        for i in range(1, 8):
            temp, txy = vs[:, i].copy(), pts[:, i].copy()
            mask = (i < n) & (vs[:, i - 1] > temp)
            pos = np.full(P, i)
            cur = mask.copy()
            for j in range(i, 0, -1):
                move = cur & (vs[:, j - 1] > temp)
                vs[move, j] = vs[move, j - 1]
                pts[move, j] = pts[move, j - 1]
                pos[move] = j - 1
                cur = move
            vs[rows[mask], pos[mask]] = temp[mask]
            pts[rows[mask], pos[mask]] = txy[mask]
        area = np.zeros(P, np.float64)
        a = pts[:, 0]
        for k in range(6):
            bb, cc = pts[:, k + 1], pts[:, k + 2]
            v = (a[:, 0] - cc[:, 0]) * (bb[:, 1] - cc[:, 1]) - (a[:, 1] - cc[:, 1]) * (bb[:, 0] - cc[:, 0])
            area = np.where(k < n - 2, area + np.abs(v.astype(np.float64) / 2.0), area)
        area1, area2 = q[:, 2] * q[:, 3], b[:, 2] * b[:, 3]
        if criterion == -1:
            r = area / ((area1 + area2).astype(np.float64) - area)
        elif criterion == 0:
            r = area / area1.astype(np.float64)
        elif criterion == 1:
            r = area / area2.astype(np.float64)
        else:
            r = area
    return r.astype(np.float32)


def rotate_iou(boxes, query_boxes, criterion=-1):
    """rotate_iou_gpu_eval: iou[n, k] = devRotateIoUEval(query_boxes[k], boxes[n], criterion), float32 [N, K]."""
    boxes, query_boxes = np.asarray(boxes, np.float32).reshape(-1, 5), np.asarray(query_boxes, np.float32).reshape(-1, 5)
    N, K = len(boxes), len(query_boxes)
    if N == 0 or K == 0:
        return np.zeros((N, K), np.float32)
    qq = np.repeat(query_boxes[None], N, 0).reshape(-1, 5)
    bb = np.repeat(boxes[:, None], K, 1).reshape(-1, 5)
    return rotate_iou_pairs(qq, bb, criterion).reshape(N, K)


# ---- eval.py overlaps ---------------------------------------------------------------------------------------------

def image_box_overlap(boxes, query_boxes, criterion=-1):
    b, q = np.asarray(boxes, np.float64)[:, None, :], np.asarray(query_boxes, np.float64)[None, :, :]
    qarea = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0])
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1])
    barea = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    if criterion == -1:
        ua = barea + qarea - iw * ih
    elif criterion == 0:
        ua = barea + 0 * qarea
    elif criterion == 1:
        ua = qarea + 0 * barea
    else:
        ua = np.ones_like(iw)
    with np.errstate(all="ignore"):
        return np.where((iw > 0) & (ih > 0), iw * ih / ua, 0.0)


def d3_box_overlap(boxes, qboxes, criterion=-1):
    boxes, qboxes = np.asarray(boxes, np.float64), np.asarray(qboxes, np.float64)
    rinc = rotate_iou(boxes[:, [0, 2, 3, 5, 6]], qboxes[:, [0, 2, 3, 5, 6]], 2)
    b, q = boxes[:, None, :], qboxes[None, :, :]
    iw = np.minimum(b[..., 1], q[..., 1]) - np.maximum(b[..., 1] - b[..., 4], q[..., 1] - q[..., 4])
    area1, area2 = b[..., 3] * b[..., 4] * b[..., 5], q[..., 3] * q[..., 4] * q[..., 5]
    inc = iw * rinc.astype(np.float64)
    ua = {-1: area1 + area2 - inc, 0: area1 + 0 * inc, 1: area2 + 0 * inc}.get(criterion, inc)
    with np.errstate(all="ignore"):
        v = np.where(iw > 0, (inc / ua).astype(np.float32), np.float32(0))
    return np.where(rinc > 0, v, rinc).astype(np.float32)


def frame_boxes(a, metric):
    if metric == 0:
        return np.asarray(a["bbox"], np.float64).reshape(-1, 4)
    if metric == 1:
        return np.concatenate([a["location"][:, [0, 2]], a["dimensions"][:, [0, 2]], a["rotation_y"][:, None]],
                              1).astype(np.float32)
    return np.concatenate([a["location"], a["dimensions"], a["rotation_y"][:, None]], 1).astype(np.float64)


def frame_overlaps(gt_annos, dt_annos, metric):
    """Per frame the reference's overlaps[f]: [n_dt, n_gt] float64 (calculate_iou_partly(dt_annos, gt_annos, metric))."""
    out = []
    for g, d in zip(gt_annos, dt_annos):
        nd, ng = len(d["name"]), len(g["name"])
        if nd == 0 or ng == 0:
            out.append(np.zeros((nd, ng)))
        elif metric == 0:
            out.append(image_box_overlap(frame_boxes(d, 0), frame_boxes(g, 0)))
        elif metric == 1:
            out.append(rotate_iou(frame_boxes(d, 1), frame_boxes(g, 1)).astype(np.float64))
        else:
            out.append(d3_box_overlap(frame_boxes(d, 2), frame_boxes(g, 2)).astype(np.float64))
    return out


# ---- compute_statistics_jit / fused_compute_statistics ------------------------------------------------------------

def _pad(frames, ovs, cd):
    F = frames.n_frames
    md, mg = max(int(frames.dt_num.max(initial=0)), 1), max(int(frames.gt_num.max(initial=0)), 1)
    dt_off = np.concatenate([[0], np.cumsum(frames.dt_num)])
    gt_off = np.concatenate([[0], np.cumsum(frames.gt_num)])
    ov = np.zeros((F, md, mg))
    igd, igg = np.full((F, md), -1, np.int8), np.full((F, mg), -1, np.int8)
    score, dta = np.zeros((F, md)), np.zeros((F, md))
    gta = np.zeros((F, mg))
    dtb = np.zeros((F, md, 4))
    for f in range(F):
        nd, ng = frames.dt_num[f], frames.gt_num[f]
        ov[f, :nd, :ng] = ovs[f]
        igd[f, :nd] = frames.ig_dt[cd, dt_off[f]:dt_off[f + 1]]
        igg[f, :ng] = frames.ig_gt[cd, gt_off[f]:gt_off[f + 1]]
        score[f, :nd] = frames.dt_score[dt_off[f]:dt_off[f + 1]]
        dta[f, :nd] = frames.dt_alpha[dt_off[f]:dt_off[f + 1]]
        dtb[f, :nd] = frames.dt_bbox[dt_off[f]:dt_off[f + 1]]
        gta[f, :ng] = frames.gt_alpha[gt_off[f]:gt_off[f + 1]]
    return ov, igd, igg, score, dta, gta, dtb


def match_scores(frames, ovs, cd, min_overlap):
    """Pass 1 (compute_fp=False): (scores, matched) [total_gt] in frame / gt order."""
    ov, igd, igg, score, _, _, _ = _pad(frames, ovs, cd)
    F, md, mg = ov.shape
    assigned = np.zeros((F, md), bool)
    out, hit = np.zeros((F, mg)), np.zeros((F, mg), bool)
    rows = np.arange(F)
    for i in range(mg):
        elig = (igd != -1) & ~assigned & (ov[:, :, i] > min_overlap) & (score > -10000000.0)
        det = np.argmax(np.where(elig, score, -np.inf), 1)
        has = elig.any(1) & (igg[:, i] != -1)
        ign = has & ((igg[:, i] == 1) | (igd[rows, det] == 1))
        tp = has & ~ign
        assigned[rows[has], det[has]] = True
        out[tp, i] = score[rows[tp], det[tp]]
        hit[tp, i] = True
    keep = np.arange(mg)[None, :] < frames.gt_num[:, None]
    return out[keep], hit[keep]


def match_pr(frames, ovs, cd, min_overlap, thresholds, metric, compute_aos, dc_ovs=None):
    """Pass 2 (compute_fp=True) for every (frame, threshold), summed over frames in order -> pr [len(thresholds), 4]."""
    assert min_overlap >= 0
    T = len(thresholds)
    if T == 0:
        return np.zeros((0, 4))
    ov, igd, igg, score, dta, gta, dtb = _pad(frames, ovs, cd)
    F, md, mg = ov.shape
    thr = np.asarray(thresholds, np.float64)[None, :, None]
    ign_thr = score[:, None, :] < thr                                    # [F, T, md]
    live = (igd != -1)[:, None, :] & ~ign_thr
    assigned = np.zeros((F, T, md), bool)
    tp, fn = np.zeros((F, T), np.int64), np.zeros((F, T), np.int64)
    sim = np.zeros((F, T))
    fi, ti = np.meshgrid(np.arange(F), np.arange(T), indexing="ij")
    for i in range(mg):
        o = np.broadcast_to(ov[:, None, :, i], (F, T, md))
        base = live & ~assigned & (o > min_overlap)
        A = base & (igd == 0)[:, None, :]
        B = base & (igd == 1)[:, None, :]
        detA = np.argmax(np.where(A, o, -np.inf), 2)
        detB = np.argmax(B, 2)
        hasA, hasB = A.any(2), B.any(2)
        det = np.where(hasA, detA, detB)
        has = (hasA | hasB)
        g = igg[:, i][:, None]
        fn += (~has & (g == 0))
        ign = has & ((g == 1) | (igd[fi, det] == 1))
        t = has & ~ign & (g != -1)
        has = has & (g != -1)
        assigned[fi[has], ti[has], det[has]] = True
        tp += t
        if compute_aos:
            term = (1.0 + np.cos(gta[:, i][:, None] - dta[fi, det])) / 2.0
            sim = np.where(t, sim + term, sim)
    fp = (~(assigned | (igd == -1)[:, None, :] | (igd == 1)[:, None, :] | ign_thr)).sum(2)
    if metric == 0 and dc_ovs is not None:
        mdc = max(max((x.shape[1] for x in dc_ovs), default=0), 1)
        dc = np.zeros((F, md, mdc))
        dcv = np.zeros((F, mdc), bool)
        for f, x in enumerate(dc_ovs):
            dc[f, :x.shape[0], :x.shape[1]] = x
            dcv[f, :x.shape[1]] = True
        nstuff = np.zeros((F, T), np.int64)
        for i in range(mdc):
            c = (~assigned & (igd == 0)[:, None, :] & ~ign_thr & (dc[:, None, :, i] > min_overlap)
                 & dcv[:, i][:, None, None])
            assigned |= c
            nstuff += c.sum(2)
        fp = fp - nstuff
    if compute_aos:
        sim = np.where((tp > 0) | (fp > 0), sim, -1.0)
    pr = np.zeros((T, 4))
    pr[:, 0], pr[:, 1], pr[:, 2] = tp.sum(0), fp.sum(0), fn.sum(0)
    pr[:, 3] = np.cumsum(np.concatenate([np.zeros((1, T)), np.where(sim != -1, sim, 0.0)], 0), 0)[-1]
    return pr


def dontcare_overlaps(frames):
    """Per frame image_box_overlap(dt bbox, DontCare bbox, 0): [n_dt, n_dc]."""
    dt_off = np.concatenate([[0], np.cumsum(frames.dt_num)])
    dc_off = np.concatenate([[0], np.cumsum(frames.dc_num)])
    return [image_box_overlap(frames.dt_bbox[dt_off[f]:dt_off[f + 1]], frames.dc_bbox[dc_off[f]:dc_off[f + 1]], 0)
            for f in range(frames.n_frames)]


class NumpyRun:
    """Stand-in for cpd_amd.kitti_eval._MetricRun: the same stages on the host."""

    def __init__(self, frames, gt_annos, dt_annos, metric, sweeps):
        self.fr, self.metric, self.sweeps = frames, metric, sweeps
        self.ovs = frame_overlaps(gt_annos, dt_annos, metric)

    def matched_scores(self):
        res = [match_scores(self.fr, self.ovs, cd, mo) for (_, _, _, cd, mo) in self.sweeps]
        return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])

    def pr(self, thresholds, compute_aos):
        dc = dontcare_overlaps(self.fr) if self.metric == 0 else None
        out = np.zeros((len(self.sweeps), N_SAMPLE_PTS, 4))
        for s, (_, _, _, cd, mo) in enumerate(self.sweeps):
            T = len(thresholds[s])
            out[s, :T] = match_pr(self.fr, self.ovs, cd, mo, thresholds[s], self.metric, compute_aos, dc)
        return out


@contextlib.contextmanager
def numpy_stages():
    from cpd_amd import kitti_eval
    saved = kitti_eval._MetricRun
    kitti_eval._MetricRun = NumpyRun
    try:
        yield kitti_eval
    finally:
        kitti_eval._MetricRun = saved


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None):
    with numpy_stages() as ke:
        return ke.get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=PR_detail_dict)


# ---- fixtures --------------------------------------------------------------------------------------------------------

def annos_from_npz(z, prefix):
    """Split the flat arrays of a golden file back into per-frame kitti_common dicts."""
    num = z[prefix + "num"]
    off = np.concatenate([[0], np.cumsum(num)])
    keys = [k[len(prefix):] for k in z.files if k.startswith(prefix) and k != prefix + "num"]
    return [{k: z[prefix + k][off[f]:off[f + 1]] for k in keys} for f in range(len(num))]


def annos_to_flat(annos, prefix):
    out = {prefix + "num": np.array([len(a["name"]) for a in annos], np.int64)}
    for k in annos[0]:
        out[prefix + k] = np.concatenate([a[k] for a in annos], 0)
    return out


def separate_from_thresholds(gt_annos, dt_annos, overlap_fns, seed=0, margin=1e-4, max_rounds=50):
    """Re-jitter, in place, every detection whose overlap with a gt (any metric, and image overlap over its own area
    with DontCare boxes) lies within `margin` of 0.25 / 0.5 / 0.7, or is NaN (a pair the reference's 8-point buffer
    cannot hold), so that APs do not hinge on the last bit of an overlap. overlap_fns(g, d) -> list of [n_dt, n_gt]."""
    rng = np.random.default_rng(seed)
    for g, d in zip(gt_annos, dt_annos):
        if len(d["name"]) == 0 or len(g["name"]) == 0:
            continue
        for _ in range(max_rounds):
            bad = np.zeros(len(d["name"]), bool)
            for o in overlap_fns(g, d):
                near = np.isnan(o)
                for m in MIN_OVERLAPS:
                    near |= np.abs(o - m) < margin
                bad |= near.any(1)
            if not bad.any():
                break
            k = int(bad.sum())
            d["bbox"][bad] += rng.normal(0, 0.5, (k, 4))
            d["location"][bad] += rng.normal(0, 0.02, (k, 3))
            d["rotation_y"][bad] += rng.normal(0, 0.01, k)
        else:
            raise RuntimeError("could not separate a frame's overlaps from the thresholds")


def numpy_overlap_fns(g, d):
    dc = g["name"] == "DontCare"
    return [image_box_overlap(d["bbox"], g["bbox"]), image_box_overlap(d["bbox"], g["bbox"][dc], 0),
            rotate_iou(frame_boxes(d, 1), frame_boxes(g, 1)), d3_box_overlap(frame_boxes(d, 2), frame_boxes(g, 2))]


def synthetic_set(n_frames, seed, margin=1e-3):
    """A seeded set whose overlaps all lie `margin` away from the thresholds: float32 rotated overlaps of the device
    and of this restatement can differ by ~1e-4 (one-ulp sin / cos differences at nearly parallel edges)."""
    from cpd_amd.synthetic import kitti_annos
    gt, dt = kitti_annos(n_frames, seed)
    separate_from_thresholds(gt, dt, numpy_overlap_fns, seed, margin=margin)
    return gt, dt
