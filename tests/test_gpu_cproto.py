"""GPU: cpd_amd.cproto (csrc/cproto.hip + the ground / DBSCAN kernels of csrc/outline.hip) against the reference's recorded
output (tests/golden/cproto.npz) and the numpy restatement (tests/ref_cproto.py) on hand-built cases whose coordinates are
exactly representable in float16."""
import copy
import os
import pickle

import numpy as np
import pytest

import ref_cproto as R
from test_cproto_ref import MG, check_stages, golden_segments, golden_sequence

pytestmark = pytest.mark.gpu
CFG = MG.golden_config()


@pytest.fixture(scope="module")
def C(hip):
    from cpd_amd import cproto
    return cproto


@pytest.fixture(scope="module")
def G(C):
    return C.CProtoGPU(CFG)


@pytest.fixture(scope="module")
def cz(golden):
    return golden("cproto")


def seg_of(res, s):
    return {k: v[s] for k, v in res.items()}


def against_restatement(G, frames, boxes, seg_frame):
    """Run the segments and compare every stage with the restatement (brute-force density: no scipy here)."""
    res = G.run(frames, boxes, seg_frame, stages=True)
    for s, (box, f) in enumerate(zip(boxes, seg_frame)):
        want = R.segment(np.asarray(frames[f])[:, 0:3], np.asarray(box, np.float64), CFG, brute=True)
        check_stages(seg_of(res, s), want, "segment %d" % s)
    return res


def cloud(rows, dtype=np.float16):
    a = np.array(rows, np.float64)
    out = a.astype(dtype)
    assert np.array_equal(out.astype(np.float64), a), "hand-built coordinates must be exact in %s" % np.dtype(dtype)
    return out


# ---- hand-built cases ----------------------------------------------------------------------------------------------------

def test_crop_order_and_strict_radius(G):
    # radius max(l, w) = 2 about (10, 5): 12.0 is exactly on it (out), one float16 step inside is in; input order is kept
    pts = cloud([[11.9921875, 5, 0.5], [30, 5, 0.5], [12, 5, 0.5], [8.5, 5, 0.25], [10, 7, 0.5], [10, 6.9921875, 0.5],
                 [10, 5, 3], [8, 5, 0.5], [10, 3.0078125, 0.5], [11.4140625, 6.4140625, 0.5], [11.421875, 6.4140625, 0.5]])
    box = [10.0, 5.0, 1.0, 2.0, 1.0, 2.0, 0.3]
    res = against_restatement(G, [pts], [box], [0])
    # (1.4140625, 1.4140625): 1.99979 < 2; (1.421875, 1.4140625): 2.0053 > 2
    np.testing.assert_array_equal(res["crop_src"][0], [0, 3, 5, 6, 8, 9])


def test_density_counts_three_and_four(G):
    step = 0.0625
    a = [[10 + step * k, 5, 0.5] for k in range(4)]                      # 4 within 0.1875 of each other: all kept
    b = [[10 + step * k, 6, 0.5] for k in range(3)]                      # 3: count 3 including itself, dropped
    c = [[10 + d, 4, 0.5] for d in (0, 0.0625, 0.125, 0.203125)]         # the ends are 0.203125 apart: they count 3, the middle 4
    pts = cloud(a + b + c)
    res = against_restatement(G, [pts], [[10.0, 5.0, 1.0, 3.0, 1.0, 2.0, 0.0]], [0])
    np.testing.assert_array_equal(res["dens_mask"][0], [1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0])
    assert res["z_min"][0] == 0.5 and res["had_points"][0]


@pytest.mark.parametrize("dtype,kept", [(np.float16, 4), (np.float32, 8)])
def test_height_window_threshold_in_the_frame_dtype(G, dtype, kept):
    # z_min = 1.5: float16(1.5) + float16(0.2) rounds to 1.7001953125, float32(1.5) + float32(0.2) = 1.70000005;
    # the rows at z = 1.7001953125 pass only the float32 frame's strict test
    zs = [1.5, 1.625, 1.7001953125, 1.75]
    pts = cloud([[10 + 0.0625 * k, 5, z] for z in zs for k in range(4)], dtype)
    assert np.float16(1.5) + 0.2 == np.float16(1.7001953125) and np.float32(1.5) + 0.2 < np.float32(1.7001953125)
    res = against_restatement(G, [pts], [[10.0, 5.0, 2.0, 1.0, 1.0, 2.0, 0.0]], [0])
    assert res["dens_mask"][0].all() and res["z_min"][0] == 1.5
    assert len(res["filt_src"][0]) == kept
    np.testing.assert_array_equal(res["new_box"][0], [10.0, 5.0, 1.5 / 2 + 1.5, 1.0, 1.0, 1.5, 0.0])


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_clamped_box_centre_in_the_frame_dtype(G, dtype):
    # z_max - z_min = 1.0 < 1.3: the reference sets h to the Python float 1.3 and numpy 2 adds h/2 = 0.65 to the z_min
    # scalar in its dtype. float16: 0.5 + float16(0.65) = 1.14990234375, a tie, rounds to 1.150390625; float32: 1.14999998
    pts = cloud([[10 + 0.0625 * k, 5, z] for z in (0.5, 0.625, 0.75) for k in range(4)], dtype)
    want = float(dtype(0.5) + 0.65)
    assert want != 1.3 / 2 + 0.5 and want == {np.float16: 1.150390625, np.float32: float(np.float32(0.65) + np.float32(0.5))}[dtype]
    res = against_restatement(G, [pts], [[10.0, 5.0, 1.0, 1.0, 1.0, 1.0, 0.0]], [0])
    assert res["had_points"][0] and res["z_min"][0] == 0.5
    np.testing.assert_array_equal(res["new_box"][0], [10.0, 5.0, want, 1.0, 1.0, 1.3, 0.0])


def test_occupancy_cell_bounds(C):
    # yaw 0, l = w = 4.5, parts 9: cells of 0.5 m with bounds exact in binary; X = x - 16, Y = y - 8
    box = np.array([16.0, 8.0, 1.0, 4.5, 4.5, 2.0, 0.0])
    P = lambda X, Y: [16 + X, 8 + Y, 1.0]
    pts = cloud([P(-2.25, -2.25), P(-2.0, -2.0),       # cell (0, 0): the lower bounds are inclusive -> 2 rows, counts
                 P(-1.75, -1.75), P(-1.5, -1.5),       # cell (1, 1): the corner belongs to the upper cell -> 2 rows, counts
                 P(-1.0, -1.0), P(-0.75, -0.75),       # cell (2, 2) holds one row, its upper corner is cell (3, 3)'s only row
                 P(2.25, 0.0), P(2.25, 0.125),          # X = l/2: the last cell's upper bound is exclusive -> in no cell
                 P(0.25, 2.0), P(0.25, 2.125)],        # cell (5, 8): 2 rows, counts
                np.float32)
    assert R.occupancy(pts, box, 9) == 3
    assert C.compute_confidence(pts, box, 9) == 3 / 81
    assert C.compute_confidence(pts[:0], box, 9) == 0.0
    want = sum(R.occupancy(pts, box, p) / p ** 2 for p in (9, 7, 5)) / 3
    assert C.hierarchical_occupancy_score(pts, box, [9, 7, 5]) == want
    css = C.CSS(CFG["RefinerConfig"]["CSSConfig"])
    assert abs(css(pts, box, "Vehicle") - R.css_from_occ([R.occupancy(pts, box, p) for p in (9, 7, 5)], box, "Vehicle",
                                                         CFG["RefinerConfig"]["CSSConfig"])) <= 1e-15
    # a rotated box with a float32 centre that is not a float64 of the box: the float32 entries are what the kernel gets
    rng = np.random.default_rng(8)
    box2 = np.array([20.3, -7.1, 0.9, 4.7, 1.9, 1.6, 0.7])
    p2 = (box2[:3] + rng.uniform(-2.2, 2.2, (300, 3)) * [1, 0.6, 0.3]).astype(np.float32)
    for parts in (9, 7, 5, 16, 1):
        assert C.compute_confidence(p2, box2, parts) == R.occupancy(p2, box2, parts) / parts ** 2


def score_direct(G, segs, min_rows=10):
    """cpd_cproto_score on hand-made non-ground rows and labels: segs = [(xyz [n, 3], labels [n], had)]."""
    import torch
    from cpd_amd.cproto import inverse_box_rows
    dev, S = G.device, len(segs)
    n = [len(x) for x, _, _ in segs]
    off = np.concatenate([[0], np.cumsum(n), [sum(n)]]).astype(np.int32)
    xyz = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x, _, _ in segs] + [np.zeros((1, 3), np.float32)])
    lab = np.concatenate([np.asarray(l, np.int32) for _, l, _ in segs] + [np.zeros(1, np.int32)])
    ncl = np.array([int(np.max(l, initial=-1)) + 1 for _, l, _ in segs] + [0], np.int32)
    boxes = np.tile(np.array([[16.0, 8.0, 1.0, 4.5, 4.5, 2.0, 0.0]]), (S, 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    idx = np.concatenate([np.arange(k) for k in n] + [np.zeros(1, int)]).astype(np.int32)
    sc = G.score(t(xyz), t(idx), t(off), t(np.array(n + [0], np.int32)), t(lab), t(ncl),
                 t(np.array([h for _, _, h in segs] + [0], np.int32)), t(idx), t(inverse_box_rows(boxes)), t(boxes), S,
                 int(sum(n)), min_rows=min_rows)
    return {k: v.cpu().numpy() for k, v in sc.items()}


def _rows(n, z=1.0):
    return [[14.0 + 0.125 * k, 8.0, z] for k in range(n)]


def test_cluster_choice_rules(G):
    segs = [
        (_rows(22), [0] * 6 + [1] * 8 + [2] * 8, 1),             # two valid clusters of equal size: the first wins
        (_rows(11), [0] * 5 + [-1] * 6, 1),                      # exactly cluster_min_points rows: rejected
        (_rows(11), [0] * 6 + [-1] * 5, 1),                      # one more: accepted
        (_rows(10), [0] * 10, 1),                                # exactly 10 non-ground rows: does not score
        (_rows(11), [0] * 11, 1),                                # 11 do
        (_rows(11), [0] * 11, 0),                                # no dense rows (had_points 0): does not score
        (_rows(10) + [[15.5, 8.0, 4.0]], [0] * 11, 1),           # max z exactly discard_max_height: rejected
        (_rows(12) + _rows(9, 2.0) + [[15.5, 8.0, 4.0]], [1] * 12 + [0] * 9 + [1], 1),   # the larger cluster is too high
    ]
    sc = score_direct(G, segs)
    np.testing.assert_array_equal(sc["best_label"][:8], [1, -1, 0, -1, 0, -1, -1, 0])
    np.testing.assert_array_equal(sc["best_count"][:8], [8, 0, 6, 0, 11, 0, 0, 9])
    np.testing.assert_array_equal(sc["out_off"], np.concatenate([[0], np.cumsum([8, 0, 6, 0, 11, 0, 0, 9])]))
    np.testing.assert_array_equal(sc["out_src"][:8], np.arange(6, 14))        # the chosen rows, in index order
    np.testing.assert_array_equal(sc["out_src"][25:34], np.arange(12, 21))
    assert (sc["occ"][[1, 3, 5, 6]] == 0).all()
    # segment 0's cluster 1 = rows 6..13: X = -1.25 .. -0.375 in steps of 0.125 -> cells 2 and 3 of 9 hold four rows each
    assert sc["occ"][0].tolist() == [R.occupancy(np.array(_rows(22)[6:14]), np.array([16.0, 8.0, 1.0, 4.5, 4.5, 2.0, 0.0]), p)
                                     for p in (9, 7, 5)]
    assert sc["occ"][0][0] == 2


def test_empty_crop_and_no_segments(G):
    pts = cloud([[10 + 0.0625 * k, 5, 0.5] for k in range(8)])
    # no rows: z_min is the box bottom, and a box lower than 1.3 m is raised to it
    res = against_restatement(G, [pts], [[40.0, 5.0, 1.0, 2.0, 1.0, 1.0, 0.0], [10.0, 5.0, 1.0, 2.0, 1.0, 2.0, 0.0]], [0, 0])
    assert len(res["crop_src"][0]) == 0 and not res["had_points"][0] and res["best_label"][0] == -1
    assert res["z_min"][0] == 0.5 and res["new_box"][0].tolist() == [40.0, 5.0, 1.3 / 2 + 0.5, 2.0, 1.0, 1.3, 0.0]
    assert len(res["crop_src"][1]) == 8
    none = G.run([pts], np.zeros((0, 7)), [], stages=True)
    assert len(none["z_min"]) == 0 and none["occ"].shape == (0, 3) and none["cluster"] == []
    far = G.run([pts], [[40.0, 5.0, 1.0, 2.0, 1.0, 2.0, 0.0]], [0])           # a chunk whose crops are all empty
    assert far["best_label"].tolist() == [-1] and len(far["cluster"][0]) == 0


def lattice_frame(seed, n, dtype=np.float16, centre=(12.0, 6.0)):
    """n rows on a 1/16 m lattice around `centre` (exact in float16), shuffled: 60 % in a dense 2 x 2 x 1 m block 1 m up
    (they survive the density filter and cluster), the rest scattered over 8 x 8 x 2.5 m."""
    rng = np.random.default_rng(seed)
    k = int(0.6 * n)
    block = np.concatenate([rng.integers(-16, 16, (k, 2)) / 16.0, 1 + rng.integers(0, 16, (k, 1)) / 16.0], 1)
    rest = np.concatenate([rng.integers(-64, 64, (n - k, 2)) / 16.0, rng.integers(0, 40, (n - k, 1)) / 16.0], 1)
    rows = np.concatenate([block, rest])[rng.permutation(n)]
    rows[:, 0:2] += np.asarray(centre)
    return cloud(rows, dtype)


def test_crop_spans_every_wave_and_many_steps(G):
    # 3000 rows, most of them inside the radius, spread over the whole frame: each of the four waves of the
    # segment's workgroup owns a quarter (768 rows = 12 steps of 64) and places its rows behind the waves before it
    pts = lattice_frame(1, 3000)
    box = [12.0, 6.0, 1.25, 3.25, 1.5, 2.5, 0.4]
    res = against_restatement(G, [pts], [box], [0])
    assert 2000 < len(res["crop_src"][0]) < 2900 and (np.diff(res["crop_src"][0]) > 0).all()
    assert len(res["filt_src"][0]) > 600 and res["best_label"][0] >= 0


def test_two_frames_keep_their_points_apart(G):
    f0, f1 = lattice_frame(2, 1500), lattice_frame(3, 1200)
    box = [12.0, 6.0, 1.25, 3.0, 1.5, 2.5, 0.0]
    both = against_restatement(G, [f0, f1], [box, box, box], [1, 0, 1])
    alone = G.run([f1], [box], [0], stages=True)
    for k in ("crop_src", "filt_src", "ng_src", "labels", "cluster_src"):
        np.testing.assert_array_equal(both[k][0], alone[k][0])
        np.testing.assert_array_equal(both[k][2], alone[k][0])
    assert not np.array_equal(both["crop_src"][0], both["crop_src"][1])


def test_sub_batch_split(C, G):
    frames = [lattice_frame(4, 1500), lattice_frame(5, 1500, centre=(13.0, 6.5))]
    boxes = [[12.0 + 0.25 * k, 6.0, 1.25, 2.5, 1.5, 2.5, 0.1 * k] for k in range(5)] + [[60.0, 6.0, 1.0, 2.0, 1.0, 2.0, 0.0]]
    seg_frame = [0, 1, 1, 0, 1, 0]
    whole = G.run(frames, boxes, seg_frame, stages=True)
    small = C.CProtoGPU(CFG, sub_batch=2)
    assert small.sub_batch == 2
    split = small.run(frames, boxes, seg_frame, stages=True)
    for k, v in whole.items():
        if isinstance(v, list):
            for a, b in zip(v, split[k]):
                np.testing.assert_array_equal(a, b, err_msg=k)
        else:
            np.testing.assert_array_equal(v, split[k], err_msg=k)
    assert (whole["best_label"][:5] >= 0).any()


def test_smooth_points_helper(C):
    pts = lattice_frame(6, 700)
    np.testing.assert_array_equal(C.smooth_points(pts), pts[R.smooth_mask_brute(pts)])
    five = lattice_frame(6, 700, np.float32)
    full = np.concatenate([five, np.ones((700, 2), np.float32)], 1)              # extra columns ride along
    np.testing.assert_array_equal(C.smooth_points(full), full[R.smooth_mask_brute(five)])
    assert len(C.smooth_points(pts[:0])) == 0


# ---- the golden sequence ---------------------------------------------------------------------------------------------------

_RUN = {}


def golden_run(C, cz, chunk=16):
    """score_frames over the golden sequence, once per chunk size: (infos, raw prototypes, [(where, stages)])."""
    if chunk not in _RUN:
        frames, infos = golden_sequence(cz)
        c = C.C_PROTO(str(cz["seq"]), "/nonexistent", CFG, chunk=chunk)
        raw, stages = {k: {} for k in C.CLASSES}, []
        c.score_frames([f[:, 0:3] for f in frames], infos, raw, stages)
        _RUN[chunk] = (infos, raw, stages)
    return _RUN[chunk]


def test_golden_every_stage(C, cz):
    _, _, stages = golden_run(C, cz)
    want = {s["where"]: s for s in golden_segments(cz)}
    seen = 0
    for where, res in stages:
        for s, w in enumerate(where):
            check_stages(seg_of(res, s), want[w], "frame %d box %d" % w)
            seen += 1
    assert seen == len(want)


def check_raw(C, raw, infos, cz):
    """Scores, boxes and raw prototypes against the golden's (the reference's, or on a flagged box the restatement's)."""
    segs = {s["where"]: s for s in golden_segments(cz)}
    for i, info in enumerate(infos):
        want = cz["info%d_score" % i].copy()
        for (fi, b), s in segs.items():
            if fi == i and s["flag"]:
                assert info["outline_score"][b] == s["score"]
                want[b] = info["outline_score"][b]
        np.testing.assert_allclose(info["outline_score"], want, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(info["outline_box"], cz["info%d_box" % i])
    ref = MG.unpack_raw(cz)
    e = 0
    for c in C.CLASSES:
        assert list(raw[c]) == list(ref[c]), c
        for pid in ref[c]:
            got, want = raw[c][pid], ref[c][pid]
            assert len(got["score"]) == len(want["score"])
            for k in range(len(want["score"])):
                flagged = segs[tuple(cz["raw_where"][e])]["flag"]
                assert abs(got["score"][k] - (segs[tuple(cz["raw_where"][e])]["score"] if flagged else want["score"][k])) <= 1e-12
                np.testing.assert_array_equal(got["outline_box"][k], want["outline_box"][k])
                np.testing.assert_array_equal(got["pose"][k], want["pose"][k])
                if k == 0:
                    np.testing.assert_array_equal(got["points"][k], want["points"][k])       # the cluster's rows, in value
                    assert got["points"][k].dtype == np.float64
                else:
                    np.testing.assert_allclose(got["points"][k], want["points"][k], rtol=0, atol=1e-9)
                np.testing.assert_allclose(got["global_position"][k], want["global_position"][k], rtol=0, atol=1e-9)
                e += 1


def test_golden_scores_and_raw_prototypes(C, cz):
    infos, raw, _ = golden_run(C, cz)
    check_raw(C, raw, infos, cz)
    protos = C.construct_prototypes(copy.deepcopy(raw), CFG["RefinerConfig"])
    got = MG.pack_proto(protos)
    for k in ("basic_key", "hq_key", "pp_key", "pp_move", "pp_n"):
        np.testing.assert_array_equal(got[k], cz[k], err_msg=k)
    np.testing.assert_allclose(got["pp_pts"], cz["pp_pts"], rtol=0, atol=1e-9)


def test_driver_files_and_cache(C, cz, tmp_path, monkeypatch):
    frames, infos = golden_sequence(cz)
    seq = str(cz["seq"])
    os.makedirs(tmp_path / seq)
    for i, f in enumerate(frames):
        np.save(tmp_path / seq / ("%04d.npy" % i), f)
    with open(tmp_path / seq / (seq + "_outline_MFCF.pkl"), "wb") as f:
        pickle.dump(infos, f)
    out = C.create_css([seq], str(tmp_path), CFG, chunk=2)[0]
    load = lambda suffix: pickle.load(open(tmp_path / seq / (seq + "_outline_MFCF" + suffix + ".pkl"), "rb"))
    saved, raw, proto = load("_CSS"), load("_CSS_raw_proto"), load("_CSS_proto")
    check_raw(C, raw, saved, cz)
    for a, b in zip(out, saved):
        np.testing.assert_array_equal(a["outline_score"], b["outline_score"])
    np.testing.assert_array_equal(MG.pack_proto(proto)["pp_key"], cz["pp_key"])
    # the second call returns the cached file and never reaches the GPU

    def no_gpu(*a, **k):
        raise AssertionError("the cached result must not launch anything")

    monkeypatch.setattr(C.CProtoGPU, "run", no_gpu)
    monkeypatch.setattr(C.CProtoGPU, "__init__", no_gpu)
    again = C.C_PROTO(seq, str(tmp_path), CFG).compute_css_score_and_raw_proto()
    for a, b in zip(again, saved):
        np.testing.assert_array_equal(a["outline_score"], b["outline_score"])
        np.testing.assert_array_equal(a["outline_box"], b["outline_box"])


def _same_raw(a, b):
    assert {c: list(a[c]) for c in a} == {c: list(b[c]) for c in b}
    for c in a:
        for pid in a[c]:
            for k in a[c][pid]:
                assert len(a[c][pid][k]) == len(b[c][pid][k])
                for x, y in zip(a[c][pid][k], b[c][pid][k]):
                    np.testing.assert_array_equal(x, y)


def test_batching_and_repetition_give_identical_output(C, cz):
    infos3, raw3, _ = golden_run(C, cz, chunk=3)
    infos1, raw1, _ = golden_run(C, cz, chunk=1)
    _RUN.pop(3)
    infos3b, raw3b, _ = golden_run(C, cz, chunk=3)            # the same run again
    for other_infos, other_raw in ((infos1, raw1), (infos3b, raw3b)):
        for a, b in zip(infos3, other_infos):
            np.testing.assert_array_equal(a["outline_score"], b["outline_score"])
            np.testing.assert_array_equal(a["outline_box"], b["outline_box"])
        _same_raw(raw3, other_raw)
    # frames 0 and 2 share a dtype: one launch sequence for both against one each
    frames, infos = golden_sequence(cz)
    sub = [frames[0][:, 0:3], frames[2][:, 0:3]]
    outs = []
    for chunk in (1, 2):
        inf = copy.deepcopy([infos[0], infos[2]])
        raw = {k: {} for k in C.CLASSES}
        C.C_PROTO(str(cz["seq"]), "/nonexistent", CFG, chunk=chunk).score_frames(sub, inf, raw)
        outs.append((inf, raw))
    for a, b in zip(outs[0][0], outs[1][0]):
        np.testing.assert_array_equal(a["outline_score"], b["outline_score"])
    _same_raw(outs[0][1], outs[1][1])
