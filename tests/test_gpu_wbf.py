"""GPU: cpd_wbf_cluster (csrc/wbf.hip, csrc/wbf_rules.h) through the C-ABI binding (cpd_amd.ops.wbf_cluster) and through cpd_amd.wbf,
against the reference's own methods (tests/golden/wbf.npz) and the numpy restatement (tests/ref_wbf.py) on generated inputs.

Every comparison is exact: the cluster of every box, the output counts, and -- the kernel reproduces numpy's float32 / float64
arithmetic op by op -- the fused boxes and scores bit for bit (the bound asked of them was one float32 ulp; `same` prints the largest
distance in ulps before it asserts equality). Exactness of the DECISIONS rests on margins: the device IoU contract is 1e-4, so every
generated input is first shown to keep every max IoU 1e-3 away from every threshold and every joining box's runner-up 1e-3 below
its maximum (`reference` asserts it before anything is compared); the one deliberate tie is between two exactly equal IoUs."""
import numpy as np
import pytest

import ref_wbf as R

pytestmark = pytest.mark.gpu
WBF_CASES = ("wbf_mean", "wbf_pi", "wbf_max", "wbf_one")
MODEL_CASES = ("model_mean_retain", "model_max_retain", "model_mean_noretain", "model_max_noretain")
MEAN, MAX, MODEL, NO_RETAIN = 0, 1, 2, 4
BLOCK, LDS_CLUSTERS = 256, 512                 # CPD_WBF_BLOCK, CPD_WBF_LDS_CLUSTERS (test_wbf_ref checks cpd_amd.wbf's copies)


@pytest.fixture(scope="module")
def wz(golden):
    return golden("wbf")


def cuda(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def ulps(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    d[both_nan] = 0
    return float(np.nan_to_num(d, nan=np.inf).max(initial=0))


def same(got, want, what):
    print("%s: %d values, largest distance %.3g ulp" % (what, np.size(want), ulps(got, want)))
    assert np.array_equal(np.asarray(got, np.float32), np.asarray(want, np.float32), equal_nan=True), what


def mode_of(kind, model=False, retain=True):
    return (MAX if kind == "max" else MEAN) | (MODEL if model else 0) | (0 if retain or not model else NO_RETAIN)


def reference(oracle, boxes, scores, start, count, thresh, mode, tie_ok=False):
    """the restatement over the segments, margins asserted -> (out_boxes, out_scores, out_count, cluster_of) laid out as the kernel's"""
    m = len(scores)
    ob, os_, cl = np.zeros((m, 7), np.float32), np.zeros(m, np.float32), np.full(m, -3, np.int32)
    oc = np.zeros(len(start), np.int32)
    for s, (a, c) in enumerate(zip(start, count)):
        kind = "max" if mode[s] & MAX else "mean"
        if mode[s] & MODEL:
            rs, rb, rc, tr = R.model_compute_wbf(scores[a:a + c], boxes[a:a + c], oracle.boxes_iou_bev, thresh[s][0], thresh[s][1], kind,
                                                 not (mode[s] & NO_RETAIN))[:4]
            ts = [thresh[s][0], thresh[s][1], 0.03]
        else:
            rs, rb, rc, tr = R.compute_wbf(scores[a:a + c], boxes[a:a + c], thresh[s][0], oracle.boxes_iou_bev, kind)
            ts = [thresh[s][0]]
        if tie_ok:
            tr = [(i, v, v - 1 if v == second else second, k, what) for i, v, second, k, what in tr]
        assert R.margins_ok(tr, ts), "segment %d: the input does not keep the margins" % s
        oc[s] = len(rs)
        ob[a:a + len(rs)], os_[a:a + len(rs)], cl[a:a + c] = rb, rs, rc
    return ob, os_, oc, cl


def launch(boxes, scores, start, count, thresh, mode):
    """cpd_wbf_cluster through cpd_amd.ops -> numpy (out_boxes, out_scores, out_count, cluster_of); rows no segment owns keep 7 / -3"""
    import torch
    from cpd_amd import ops
    m = len(scores)
    ob = torch.full((m, 7), 7.0, device="cuda")
    os_ = torch.full((m,), 7.0, device="cuda")
    got = ops.wbf_cluster(cuda(boxes).reshape(-1, 7), cuda(scores), cuda(start, np.int32), cuda(count, np.int32), cuda(thresh).reshape(-1, 2),
                          cuda(mode, np.int32), out_boxes=ob, out_scores=os_)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in got)


def compare(got, want, start, what):
    """segment by segment: counts and clusters exact, the written rows bit for bit, rows past a segment's count untouched"""
    gb, gs, gc, gl = got
    wb, ws, wc, wl = want
    assert np.array_equal(gc, wc), what
    assert np.array_equal(gl, wl), what
    rows = np.zeros(len(gs), bool)
    for a, k in zip(start, wc):
        rows[a:a + k] = True
    same(gb[rows], wb[rows], what + " boxes")
    same(gs[rows], ws[rows], what + " scores")
    assert (gb[~rows] == 7.0).all() and (gs[~rows] == 7.0).all(), what + ": a row outside the results was written"


def one_segment(scores, boxes, thresh, mode, thresh2=0.0):
    n = len(scores)
    return (np.asarray(boxes, np.float32).reshape(-1, 7), np.asarray(scores, np.float32), np.zeros(1, np.int32), np.array([n], np.int32),
            np.array([[thresh, thresh2]], np.float32), np.array([mode], np.int32))


def golden_segment(wz, name):
    model = name.startswith("model")
    mode = mode_of(str(wz[name + "_type"]), model, bool(wz[name + "_retain"]) if model else True)
    return one_segment(wz[name + "_scores"], wz[name + "_boxes"], float(wz[name + "_thresh"]), mode, float(wz[name + "_thresh2"]) if model else 0.0)


# ---- the reference's own results ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", WBF_CASES + MODEL_CASES)
def test_golden_through_the_abi_and_the_python_layer(hip, wz, oracle, name):
    import torch
    from cpd_amd import wbf
    seg = golden_segment(wz, name)
    want = reference(oracle, *seg)
    got = launch(*seg)
    compare(got, want, seg[2], name)
    k = len(wz[name + "_out_scores"])
    assert got[2][0] == k and np.array_equal(got[3], wz[name + "_cluster_of"])
    same(got[0][:k], wz[name + "_out_boxes"], name + " boxes against the reference's")
    same(got[1][:k], wz[name + "_out_scores"], name + " scores against the reference's")
    names = np.array(["n%d" % i for i in range(len(seg[1]))])
    s, b = seg[1].copy(), seg[0].copy()
    if name.startswith("model"):
        args = (float(wz[name + "_thresh"]), float(wz[name + "_thresh2"]), str(wz[name + "_type"]), bool(wz[name + "_retain"]))
        fn = wbf.model_compute_WBF
        cl = wz[name + "_cluster_of"]
        want_names = names[cl == R.SINGLE].tolist() + names[[np.flatnonzero(cl == c)[0] for c in range(cl.max() + 1)]].tolist()
    else:
        args = (float(wz[name + "_thresh"]), str(wz[name + "_type"]))
        fn = wbf.compute_WBF
        want_names = names[:k].tolist()
    gn, gs, gb = fn(names, s, b, *args)
    assert gn.tolist() == want_names
    same(gs, wz[name + "_out_scores"], name + " python scores")
    same(gb, wz[name + "_out_boxes"], name + " python boxes")
    assert np.array_equal(s, seg[1]) and np.array_equal(b, seg[0])                    # the caller's arrays stay as they were
    ts, tb = cuda(s), cuda(b)
    gn, gs, gb = fn(names, ts, tb, *args)                                             # device tensors in, device tensors out
    assert gs.is_cuda and gb.is_cuda and torch.equal(ts.cpu(), torch.from_numpy(s)) and torch.equal(tb.cpu(), torch.from_numpy(b))
    same(gs.cpu().numpy(), wz[name + "_out_scores"], name + " tensor scores")
    same(gb.cpu().numpy(), wz[name + "_out_boxes"], name + " tensor boxes")


def test_merge_golden_on_the_device(hip, wz):
    """merge_by_WBF per frame and merge_frames over all frames (one launch), the NMS class through nms_gpu"""
    from cpd_amd import wbf
    cfg = {"WBF_IOUS": list(wz["merge_cfg_WBF_IOUS"]), "WBF_PRE_SCORES": list(wz["merge_cfg_WBF_PRE_SCORES"]),
           "MERGE_TYPE": [str(t) for t in wz["merge_cfg_MERGE_TYPE"]], "NMS_IOU": float(wz["merge_cfg_NMS_IOU"])}
    classes = tuple(str(c) for c in wz["merge_classes"])
    cut, ocut = np.cumsum([0] + list(wz["merge_n"])), np.cumsum([0] + list(wz["merge_out_n"]))
    frames = [(wz["merge_names"][a:b], wz["merge_scores"][a:b], wz["merge_boxes"][a:b]) for a, b in zip(cut[:-1], cut[1:])]
    for f, (n, s, b) in enumerate(frames):
        gn, gs, gb = wbf.merge_by_WBF(n, s, b, cfg, classes)
        assert np.array_equal(gn, wz["merge_out_names"][ocut[f]:ocut[f + 1]])
        same(gs, wz["merge_out_scores"][ocut[f]:ocut[f + 1]], "merge frame %d scores" % f)
        same(gb, wz["merge_out_boxes"][ocut[f]:ocut[f + 1]], "merge frame %d boxes" % f)
    views = [[{"name": n[v::2], "score": s[v::2], "boxes_lidar": b[v::2], "frame_id": f} for f, (n, s, b) in enumerate(frames)] for v in range(2)]
    out = wbf.merge_frames(views, cfg, classes)
    assert [o["frame_id"] for o in out] == [0, 1, 2]
    assert np.array_equal(np.concatenate([o["name"] for o in out]), wz["merge_out_names"])    # (distinct scores: the split changes no order)
    same(np.concatenate([o["score"] for o in out]), wz["merge_out_scores"], "merge_frames scores")
    same(np.concatenate([o["boxes_lidar"] for o in out]), wz["merge_out_boxes"], "merge_frames boxes")


# ---- shapes at which the kernel can go wrong ------------------------------------------------------------------------------------------

def grid_boxes(k, rng, spacing=12.0):
    """k well separated boxes: every pair far beyond both half diagonals"""
    side = int(np.ceil(np.sqrt(k)))
    b = np.zeros((k, 7), np.float32)
    b[:, 0] = (np.arange(k) % side) * spacing + rng.uniform(-1, 1, k)
    b[:, 1] = (np.arange(k) // side) * spacing + rng.uniform(-1, 1, k)
    b[:, 2] = rng.uniform(-1, 1, k)
    b[:, 3:6] = np.array([4.7, 2.1, 1.7]) * np.exp(rng.normal(0, 0.1, (k, 3)))
    b[:, 6] = rng.uniform(-4, 4, k)
    return b


def nudged(b, rng, rel=0.03):
    v = b.astype(np.float64).copy()
    v[:2] += rng.normal(0, 1, 2) * rel * 2.0
    v[3:6] *= np.exp(rng.normal(0, rel, 3))
    v[6] += rng.normal(0, rel)
    return v.astype(np.float32)


def descending(n, hi=0.95, lo=0.1):
    return np.linspace(hi, lo, n).astype(np.float32) if n > 1 else np.full(n, hi, np.float32)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_segments(hip, oracle, n):
    rng = np.random.default_rng(n)
    base = grid_boxes(1, rng)
    boxes = np.array([nudged(base[0], rng) for _ in range(n)], np.float32).reshape(-1, 7)
    for mode, thr2 in ((MEAN, 0.0), (MAX, 0.0), (MODEL, 0.5), (MODEL | MAX | NO_RETAIN, 0.5)):
        seg = one_segment(descending(n), boxes, 0.6, mode, thr2)
        want = reference(oracle, *seg)
        compare(launch(*seg), want, seg[2], "%d boxes, mode %d" % (n, mode))
        assert want[2][0] == min(n, 1)                                                # two nudged views of one object fuse


@pytest.mark.parametrize("k", [63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, LDS_CLUSTERS - 1, LDS_CLUSTERS, LDS_CLUSTERS + 1, LDS_CLUSTERS + 70])
def test_cluster_count_across_wave_block_and_lds(hip, oracle, k):
    """k single-box clusters, then boxes that join the last, the first and (beyond the LDS-resident clusters) the last again: the
    argmax crosses waves and the block's stride, and cluster state past CPD_WBF_LDS_CLUSTERS lives in the workspace"""
    rng = np.random.default_rng(k)
    base = grid_boxes(k, rng)
    tail = [nudged(base[k - 1], rng), nudged(base[0], rng), nudged(base[k - 1], rng), nudged(base[k // 2], rng)]
    boxes = np.concatenate([base, np.array(tail, np.float32)])
    for mode, thr, thr2 in ((MEAN, 0.5, 0.0), (MODEL | MEAN, 0.6, 0.3)):
        seg = one_segment(descending(len(boxes)), boxes, thr, mode, thr2)
        want = reference(oracle, *seg)
        assert want[2][0] == k and want[3][k:].tolist() == [k - 1, 0, k - 1, k // 2]
        compare(launch(*seg), want, seg[2], "%d clusters, mode %d" % (k, mode))


@pytest.mark.parametrize("other", [1, 64, BLOCK])
def test_equal_ious_take_the_lower_index(hip, oracle, other):
    """Clusters 0 and `other` mirror each other about the joining box (dyadic coordinates, heading 0: both IoUs are the same
    float32), everything between is far away: np.argmax takes the first maximum, so the box joins cluster 0."""
    rng = np.random.default_rng(other)
    left = np.array([-1.25, 0, 0, 4, 2, 1.5, 0], np.float32)
    right = np.array([1.25, 0, 0, 4, 2, 1.5, 0], np.float32)
    mid = np.array([0, 0, 0, 4, 2, 1.5, 0], np.float32)
    far = grid_boxes(other - 1, rng) + np.array([40, 40, 0, 0, 0, 0, 0], np.float32)
    boxes = np.concatenate([left[None], far, right[None], mid[None]]).astype(np.float32)
    v = oracle.boxes_iou_bev(mid[None], np.stack([left, right]))[0]
    assert v[0] == v[1] and v[0] > 0.5 and oracle.boxes_iou_bev(left[None], right[None])[0, 0] < 0.25
    for mode in (MEAN, MAX):
        seg = one_segment(descending(len(boxes)), boxes, 0.3, mode)
        want = reference(oracle, *seg, tie_ok=True)
        assert want[3][-1] == 0 and want[3][-2] == other
        compare(launch(*seg), want, seg[2], "tie with cluster %d, mode %d" % (other, mode))


def chain(rng, n, rel):
    b = np.array([3.0, -2.0, 0.3, 4.7, 2.1, 1.7, 3.1])
    bx = np.tile(b, (n, 1))
    bx[:, :2] += rng.normal(0, rel, (n, 2))
    bx[:, 3:6] *= np.exp(rng.normal(0, rel * 0.3, (n, 3)))
    bx[:, 6] += rng.normal(0, rel * 2, n)
    return np.sort(rng.uniform(0.1, 0.95, n))[::-1].astype(np.float32), bx.astype(np.float32)


@pytest.mark.parametrize("n,mode,rel", [(40, MEAN, 0.15), (40, MAX, 0.15), (9, MODEL, 0.004), (130, MODEL, 0.004), (300, MODEL | NO_RETAIN, 0.004)])
def test_one_long_cluster(hip, oracle, n, mode, rel):
    """40 members drifting in WBF-mean (every join re-sums the chain from the merged box); in the model variant 9, 130 and 300
    members: numpy's pairwise float32 sum of the heading residuals takes its three paths (short, one block, split halves)"""
    scores, boxes = chain(np.random.default_rng(n + mode), n, rel)
    seg = one_segment(scores, boxes, 0.9 if mode & MODEL else 0.3, mode, 0.5)
    want = reference(oracle, *seg)
    assert want[2][0] == 1 and (want[3] == 0).all()
    compare(launch(*seg), want, seg[2], "%d members, mode %d" % (n, mode))


def mixed_batch(oracle, n_seg, seed):
    """n_seg segments of mixed sizes (empty ones included) and modes, with unused rows between some of them; every segment is
    drawn again until it keeps the margins"""
    modes = [(MEAN, 0.55, 0.0), (MAX, 0.4, 0.0), (MODEL, 0.9, 0.5), (MODEL | MAX, 0.8, 0.4), (MODEL | NO_RETAIN, 0.85, 0.5),
             (MODEL | MAX | NO_RETAIN, 0.9, 0.5)]
    boxes, scores, start, count, thresh, mode = [], [], [], [], [], []
    at = 0
    for s in range(n_seg):
        m, thr, thr2 = modes[s % len(modes)]
        n_obj = [0, 1, 3, 8, 14][s % 5]
        for attempt in range(50):
            rng = np.random.default_rng(seed * 1000 + s * 50 + attempt)
            if n_obj == 0:
                sc, bx = np.zeros(0, np.float32), np.zeros((0, 7), np.float32)
            else:
                _, sc, bx = R.gen_detections(rng, n_obj, classes=("Car",), jitter=2.0 if m & MODEL else 1.0, n_isolated=s % 3, n_low=0)
                sc, bx = R.sorted_segment(sc, bx)
            tr = (R.model_compute_wbf(sc, bx, oracle.boxes_iou_bev, thr, thr2, "max" if m & MAX else "mean", not (m & NO_RETAIN))[3] if m & MODEL
                  else R.compute_wbf(sc, bx, thr, oracle.boxes_iou_bev, "max" if m & MAX else "mean")[3])
            if R.margins_ok(tr, [thr, thr2, 0.03] if m & MODEL else [thr]):
                break
        else:
            raise AssertionError("no draw of segment %d keeps the margins" % s)
        gap = s % 4 == 1                                                              # two rows no segment owns
        boxes += [bx] + ([np.full((2, 7), 3.0, np.float32)] if gap else [])
        scores += [sc] + ([np.full(2, 0.5, np.float32)] if gap else [])
        start.append(at)
        count.append(len(sc))
        thresh.append((thr, thr2))
        mode.append(m)
        at += len(sc) + (2 if gap else 0)
    return (np.concatenate(boxes), np.concatenate(scores), np.array(start, np.int32), np.array(count, np.int32), np.array(thresh, np.float32),
            np.array(mode, np.int32))


@pytest.fixture(scope="module")
def batch37(oracle):
    seg = mixed_batch(oracle, 37, 1)
    return seg, reference(oracle, *seg)


def test_one_launch_of_37_segments_equals_37_launches(hip, batch37):
    seg, want = batch37
    boxes, scores, start, count, thresh, mode = seg
    assert (count == 0).sum() >= 7 and count.max() > 40 and len(set(mode.tolist())) == 6
    got = launch(*seg)
    compare(got, want, start, "37 segments")
    gb, gs, gc, gl = (np.full_like(got[0], 7.0), np.full_like(got[1], 7.0), np.zeros_like(got[2]), np.full_like(got[3], -3))
    for s in range(len(start)):
        one = launch(boxes, scores, start[s:s + 1], count[s:s + 1], thresh[s:s + 1], mode[s:s + 1])
        a, c, k = start[s], count[s], one[2][0]
        gb[a:a + k], gs[a:a + k], gc[s], gl[a:a + c] = one[0][a:a + k], one[1][a:a + k], k, one[3][a:a + c]
    for x, y in zip(got, (gb, gs, gc, gl)):
        assert x.tobytes() == y.tobytes()                                             # bit for bit, untouched rows included
    from cpd_amd import wbf
    host = wbf.cluster_segments_host(*seg)                                            # the same rules compiled for the host
    assert np.array_equal(host[2], got[2]) and np.array_equal(host[3], got[3])
    rows = got[1] != 7.0
    assert host[0][rows].tobytes() == got[0][rows].tobytes() and host[1][rows].tobytes() == got[1][rows].tobytes()


def test_two_streams_give_the_sequential_results(hip, oracle, batch37):
    import torch
    from cpd_amd import ops
    seg_a, want_a = batch37
    seg_b = mixed_batch(oracle, 11, 2)
    want_b = reference(oracle, *seg_b)

    def device(seg):
        b, s, st, ct, th, md = seg
        return [cuda(b).reshape(-1, 7), cuda(s), cuda(st, np.int32), cuda(ct, np.int32), cuda(th).reshape(-1, 2), cuda(md, np.int32)]

    da, db = device(seg_a), device(seg_b)
    seq_a = [t.clone() for t in ops.wbf_cluster(*da)]
    seq_b = [t.clone() for t in ops.wbf_cluster(*db)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        par_a = ops.wbf_cluster(*da)
    with torch.cuda.stream(s2):
        par_b = ops.wbf_cluster(*db)
    torch.cuda.synchronize()
    for seq, par, want, seg in ((seq_a, par_a, want_a, seg_a), (seq_b, par_b, want_b, seg_b)):
        for x, y in zip(seq, par):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert np.array_equal(par[2].cpu().numpy(), want[2]) and np.array_equal(par[3].cpu().numpy(), want[3])


def test_refused_segments_and_bad_arguments(hip):
    import torch
    from cpd_amd import _lib, ops, wbf
    lib, P = _lib.lib(), _lib.ptr
    n = wbf.MAX_SEGMENT + 1
    boxes, scores = torch.zeros(n, 7).cuda(), torch.linspace(0.9, 0.1, n).cuda()
    boxes[:, 3:6] = 1.0
    start = torch.tensor([0, 4, n - 2, 0], dtype=torch.int32).cuda()
    count = torch.tensor([n, 2, 3, -1], dtype=torch.int32).cuda()                    # too long; fine; past the end; negative
    thresh = torch.tensor([[0.5, 0.0]] * 4).cuda()
    mode = torch.zeros(4, dtype=torch.int32).cuda()
    ob, os_, oc, cl = ops.wbf_cluster(boxes, scores, start, count, thresh, mode)
    torch.cuda.synchronize()
    assert oc.tolist() == [-1, 1, -1, -1]                                            # never truncated: refused whole
    assert cl[4:6].tolist() == [0, 0] and (cl[:4] == -3).all() and (cl[6:] == -3).all() and not ob[6:].any()
    with pytest.raises(ValueError):
        wbf.cluster_segments(boxes.cpu().numpy(), scores.cpu().numpy(), np.zeros(1, np.int32), np.array([n], np.int32),
                             np.array([[0.5, 0]], np.float32), np.zeros(1, np.int32))
    ws = torch.empty(ops.wbf_workspace_bytes(n), dtype=torch.uint8).cuda()
    args = (P(boxes), P(scores), n, P(start), P(count), P(thresh), P(mode), 4, P(ob), P(os_), P(oc), P(cl))
    assert lib.cpd_wbf_cluster(*args, P(ws), ws.numel() - 256, _lib.stream()) == -2   # CPD_ERR_WORKSPACE
    assert lib.cpd_wbf_cluster(*args, None, 0, _lib.stream()) == -2
    assert lib.cpd_wbf_cluster(None, *args[1:], P(ws), ws.numel(), _lib.stream()) == -1   # CPD_ERR_ARG
    assert lib.cpd_wbf_cluster(*args[:3], None, *args[4:], P(ws), ws.numel(), _lib.stream()) == -1
    assert lib.cpd_wbf_cluster(*args[:7], 0, *args[8:], None, 0, _lib.stream()) == 0   # no segment: nothing to do
    assert ops.wbf_workspace_bytes(0) > 0 and ops.wbf_workspace_bytes(1000) >= 1000 * 26 * 4
    torch.cuda.synchronize()
