"""GPU: cpd_amd.cproto_refine (csrc/cproto_refine.hip on top of the first stage's kernels) against the numpy restatement
(tests/ref_cproto_refine.py) on hand-built clusters whose coordinates are exactly representable, and against the reference's
recorded output (tests/golden/cproto_refine.npz)."""
import copy
import os
import pickle

import numpy as np
import pytest

import ref_cproto_refine as RR
from test_cproto_refine_ref import CFG, check_final, check_resize, flagged, golden_inputs, restated

pytestmark = pytest.mark.gpu
PREDEFINED = CFG["RefinerConfig"]["CSSConfig"]["PredifinedSize"]


@pytest.fixture(scope="module")
def C(hip):
    from cpd_amd import cproto_refine
    return cproto_refine


@pytest.fixture(scope="module")
def G(C):
    return C.RefineGPU(CFG)


@pytest.fixture(scope="module")
def rz(golden):
    return golden("cproto_refine")


# ---- cpd_refine_fit_size ---------------------------------------------------------------------------------------------------------

def fit_direct(C, G, proto_set, boxes, cls, basic):
    import torch
    G.set_prototypes(C.PrototypeTable(proto_set, PREDEFINED))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(G.device)
    S = len(boxes)
    nb = t(np.array(boxes, np.float64).reshape(-1, 7) if S else np.zeros((1, 7)), np.float64)
    fit = G.fit_size(nb, t(cls if S else [0], np.int32), t(np.array(basic).reshape(-1, 3) if S else np.zeros((1, 3)), np.float64), S)
    return nb.cpu().numpy()[:S], fit.cpu().numpy()[:S]


def _protos(veh_h=(), ped_h=()):
    hq = {c: {} for c in RR.CLASSES}
    for k, h in enumerate(veh_h):
        hq['Vehicle'][700 + k] = {'box': np.array([0, 0, 0, 4.0 + k, 1.5 + 0.125 * k, h, 0.0])}
    for k, h in enumerate(ped_h):
        hq['Pedestrian'][800 + k] = {'box': np.array([0, 0, 0, 0.5 + k, 0.75, h, 0.0])}
    return {'basic_proto_set': {c: {} for c in RR.CLASSES}, 'high_quality_proto_set': hq}


def test_fit_size_kinds_ties_and_classes(C, G):
    nan = [np.nan] * 3
    box = lambda l, w, h: [10.0, 5.0, 1.0, l, w, h, 0.25]
    # Vehicle prototypes of height 1.5, 2.0, 1.0, 2.0; no Cyclist prototype
    proto = _protos(veh_h=(1.5, 2.0, 1.0, 2.0), ped_h=(1.75,))
    boxes = [box(4.5, 2.0, 1.75),      # |dh| = 0.25, 0.25, 0.75, 0.25: a tie, the first minimum wins -> 0
             box(4.5, 2.0, 1.875),     # 0.375, 0.125, 0.875, 0.125 -> 1, not 3
             box(4.5, 2.0, 1.3),       # its own basic prototype
             box(1.0, 1.0, 1.7),       # a Pedestrian with a prototype: fit_index 0, l and w kept
             box(1.9, 0.85, 1.6),      # a Cyclist: no prototype of the class -> predefined, l and w kept
             box(2.0, 0.5, 1.6)]       # a Pedestrian with its own basic prototype: l and w kept
    cls = [0, 0, 0, 1, 2, 1]
    basic = [nan, nan, [4.25, 1.75, 1.5], nan, nan, [0.5, 0.5, 1.5]]
    got, fit = fit_direct(C, G, proto, boxes, cls, basic)
    np.testing.assert_array_equal(fit, [0, 1, -2, 0, -1, -2])
    want = np.array(boxes)
    want[0, 3:5], want[1, 3:5], want[2, 3:5] = [4.0, 1.5], [5.0, 1.625], [4.25, 1.75]
    np.testing.assert_array_equal(got, want)
    for s in range(len(boxes)):        # and the restatement
        name = RR.CLASSES[cls[s]]
        bs = {c: {} for c in RR.CLASSES}
        if not np.isnan(basic[s][0]):
            bs[name][5] = np.array(basic[s])
        _, hq = RR.hq_tables(proto)
        fb, _, k = RR.fit_size(np.array(boxes[s]), name, 5, bs, hq[name][0], hq[name][1], PREDEFINED)
        assert k == fit[s] and np.array_equal(fb, got[s])


def test_fit_size_without_prototypes_and_without_segments(C, G):
    nan = [np.nan] * 3
    boxes = [[10.0, 5.0, 1.0, 4.5, 2.0, 1.75, 0.0], [10.0, 5.0, 1.0, 0.5, 0.5, 1.75, 0.0]]
    got, fit = fit_direct(C, G, _protos(), boxes, [0, 1], [nan, nan])             # hq_count = 0 for every class
    np.testing.assert_array_equal(fit, [-1, -1])
    np.testing.assert_array_equal(got, [[10.0, 5.0, 1.0, 5.065, 1.86, 1.75, 0.0], boxes[1]])
    got, fit = fit_direct(C, G, _protos(veh_h=(1.5,)), [], [], [])                # S = 0
    assert got.shape == (0, 7) and fit.shape == (0,)


# ---- cpd_refine_orient_drift on hand-made clusters ------------------------------------------------------------------------------

BOX0 = np.array([16.0, 8.0, 1.0, 4.5, 2.0, 1.5, 0.0])      # yaw 0: X = x - 16, Y = y - 8, exact


def orient_direct(G, segs):
    """cpd_refine_orient_drift on hand-made clusters: segs = [(xyz [n, 3], box [7], best_label)]."""
    import torch
    from cpd_amd.cproto import inverse_box_rows
    S = len(segs)
    n = [len(x) for x, _, _ in segs]
    xyz = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x, _, _ in segs] + [np.zeros((1, 3), np.float32)])
    for x, _, _ in segs:
        assert np.array_equal(np.asarray(x, np.float32).astype(np.float64), np.asarray(x, np.float64)), "float32 coordinates"
    boxes = np.array([b for _, b, _ in segs], np.float64).reshape(-1, 7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(G.device)
    od = G.orient_drift(t(xyz), t(np.concatenate([[0], np.cumsum(n)]).astype(np.int32)),
                        t(np.array([l for _, _, l in segs], np.int32)), t(boxes), t(inverse_box_rows(boxes)), S, int(sum(n)))
    return {k: v.cpu().numpy()[:S] for k, v in od.items()}


def check_against_restatement(got, segs, exact_xy, tol=1e-4):
    """The three boxes of every segment against the restatement: z, l, w, h bit for bit, yaw <= 1e-12, x and y bit for bit where
    the yaw is 0 (exact_xy) and within tol otherwise. Returns the worst difference per segment."""
    worst = []
    for s, (xyz, box, label) in enumerate(segs):
        box = np.asarray(box, np.float64)
        if label < 0:
            for k in ("box_drift", "box_orient", "box_orient_drift"):
                np.testing.assert_array_equal(got[k][s], box, err_msg="segment %d %s" % (s, k))
            worst.append(0.0)
            continue
        pts = np.asarray(xyz, np.float64)
        orient = RR.correct_orientation(pts, box)
        want = dict(box_drift=RR.density_guided_drift(pts, box), box_orient=orient,
                    box_orient_drift=RR.density_guided_drift(pts, orient))
        w = 0.0
        for k, v in want.items():
            what = "segment %d %s: %r vs %r" % (s, k, got[k][s], v)
            assert np.array_equal(got[k][s][2:6], v[2:6]), what
            assert abs(got[k][s][6] - v[6]) <= 1e-12, what
            if exact_xy and k != "box_orient_drift":
                assert np.array_equal(got[k][s][0:2], v[0:2]), what
            assert np.abs(got[k][s] - v).max() <= tol, what
            w = max(w, float(np.abs(got[k][s] - v).max()))
        worst.append(w)
    return worst


def P(rows):
    """Box-frame (X, Y) rows of BOX0 as sweep coordinates."""
    return [[16.0 + X, 8.0 + Y, 1.0] for X, Y in rows]


def lattice_cluster(seed, n):
    """n rows on a 1/16 m lattice in a 4 x 1.75 m footprint around BOX0's centre, off-centre so that the sides differ: many rows
    share a coordinate, so the bins see ties."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-30, 34, n) / 16.0
    Y = rng.integers(-10, 18, n) / 16.0 + (X > 0) * 0.25
    return P(zip(X, Y))


@pytest.mark.parametrize("n", [6, 64, 65, 3000])      # under one wave, a full wave, a wave plus one, many steps per wave
def test_cluster_sizes(G, n):
    segs = [(lattice_cluster(n, n), BOX0, 0), (lattice_cluster(n + 1, n), BOX0 + [0.25, -0.5, 0, 0, 0, 0, 0], 0)]
    got = orient_direct(G, segs)
    check_against_restatement(got, segs, exact_xy=True)
    if n >= 64:
        assert got["box_orient"][0][6] != 0.0 and not np.array_equal(got["box_drift"][0][0:2], BOX0[0:2])


def test_no_cluster_returns_the_box(G):
    box = np.array([20.3, -7.1, 0.9, 4.7, 1.9, 1.6, 0.7])
    segs = [(lattice_cluster(1, 40), BOX0, 0), (lattice_cluster(2, 30), box, -1), ([], box, -1), (lattice_cluster(3, 20), BOX0, 0)]
    got = orient_direct(G, segs)
    check_against_restatement(got, segs, exact_xy=True)
    for k in got:
        np.testing.assert_array_equal(got[k][1], box)
        np.testing.assert_array_equal(got[k][2], box)


def test_bin_bounds_ties_and_halves(G):
    # x branch: X from -3.5 to 3.5 -> mid 0, delta 0.5; every Y > 0 -> argmax. Rows:
    rows = [(-3.5, 1.0),       # 0: the row at min lies in no bin (its Y would win bottom bin 0)
            (3.5, 0.25),       # 1: max lies on the last top bin's upper bound: inside it
            (0.0, 5.0),        # 2: exactly at mid: in neither half (its Y would win any bin)
            (0.5, 0.5),        # 3: on top bin 0's upper bound: inside bin 0, alone there
            (0.75, 0.25),      # 4: top bin 1
            (1.0, 0.75),       # 5: on top bin 1's upper bound: inside bin 1, where it wins; bin 2 stays empty
            (-3.25, 0.5),      # 6: bottom bin 0, ties with row 7: the lower row wins
            (-3.125, 0.5),     # 7
            (-1.0, 0.25),      # 8: on bottom bin 4's upper bound (-1.5, -1]
            (-1.25, 0.125),    # 9: bottom bin 4, loses to row 8
            (-0.25, 0.375)]    # 10: bottom bin 6 (-0.5, 0]
    box = BOX0.copy()
    info = {}
    want = RR.correct_orientation(np.array(P(rows)), box, info=info)
    assert info == dict(branch='x', side='max', top=[3, 5, 1], bot=[6, 8, 10])
    top, bot = np.mean([rows[r] for r in (3, 5, 1)], 0), np.mean([rows[r] for r in (6, 8, 10)], 0)
    assert abs(want[6] - np.arctan((top[1] - bot[1]) / (top[0] - bot[0]))) <= 1e-15 and want[6] != 0.0
    # the same rows with the tie's order swapped pick row 6 again, now the other X: the yaw must differ
    swapped = list(rows)
    swapped[6], swapped[7] = rows[7], rows[6]
    segs = [(P(rows), box, 0), (P(swapped), box, 0)]
    got = orient_direct(G, segs)
    check_against_restatement(got, segs, exact_xy=True)
    assert got["box_orient"][0][6] != got["box_orient"][1][6]


def test_exactly_half_positive_takes_the_min_side(G):
    # 8 rows, 4 with Y > 0 (one Y is 0: not positive) and 4 with X > 0: neither count is more than half
    rows = [(-2.0, 0.5), (-1.5, -0.25), (-0.5, 0.75), (-1.0, 0.0), (0.5, -0.5), (1.0, 0.25), (1.5, -0.75), (2.0, 0.5)]
    info = {}
    RR.correct_orientation(np.array(P(rows)), BOX0, info=info)
    assert info["branch"] == 'x' and info["side"] == 'min'
    segs = [(P(rows), BOX0, 0), (P(rows + [(0.25, 0.125)]), BOX0, 0)]            # one more positive row: the max side
    RR.correct_orientation(np.array(segs[1][0]), BOX0, info=info)
    assert info["side"] == 'max'
    got = orient_direct(G, segs)
    check_against_restatement(got, segs, exact_xy=True)
    # drift: new_x = -l/2 - min_x, centre = -new_x; likewise y
    np.testing.assert_array_equal(got["box_drift"][0][0:2], [16.0 + (4.5 / 2 - 2.0), 8.0 + (2.0 / 2 - 0.75)])
    np.testing.assert_array_equal(got["box_drift"][1][0:2], [16.0 - (4.5 / 2 - 2.0), 8.0 - (2.0 / 2 - 0.75)])


def test_empty_halves_leave_the_yaw(G):
    # six rows at one place: the y branch (0 > 0 is false), mid = min = max, no row above or below it
    box = BOX0 + [0, 0, 0, 0, 0, 0, 0.5]
    segs = [(P([(0.5, 0.25)] * 6), BOX0, 0), ([[16.5, 8.25, 1.0]] * 6, box, 0)]
    got = orient_direct(G, segs)
    check_against_restatement(got, segs, exact_xy=False)
    assert got["box_orient"][0][6] == 0.0 and got["box_orient"][1][6] == 0.5
    np.testing.assert_array_equal(got["box_orient_drift"], got["box_drift"])     # the same box, the same inverse rows


def test_branch_test_at_equality(G):
    # l = 4, w = 2, extent 2 x 2: (2 / 4) * 2 == 2 / 2, not greater -> the y branch; a longer extent -> the x branch
    box = np.array([16.0, 8.0, 1.0, 4.0, 2.0, 1.5, 0.0])
    rows = [(-1.0, -1.0), (-0.5, 0.25), (0.25, 1.0), (1.0, 0.5), (0.5, -0.75), (-0.75, 0.75), (0.75, 0.125), (0.125, -0.5)]
    longer = [(-1.0625, -1.0)] + rows[1:]
    info = {}
    RR.correct_orientation(np.array(P(rows)), box, info=info)
    assert info["branch"] == 'y'
    by_y = RR.correct_orientation(np.array(P(rows)), box)[6]
    RR.correct_orientation(np.array(P(longer)), box, info=info)
    assert info["branch"] == 'x'
    segs = [(P(rows), box, 0), (P(longer), box, 0)]
    got = orient_direct(G, segs)
    check_against_restatement(got, segs, exact_xy=True)
    assert got["box_orient"][0][6] != got["box_orient"][1][6] and abs(got["box_orient"][0][6] - by_y) <= 1e-12


def car_cluster(rng, box, n):
    """An L-shaped car outline seen from one side: rows along one long and one short side of a footprint a little smaller than
    the box, 2 cm of noise, rotated and moved to the box. The long side spans more than 3 m, so the means of the picked rows of
    the two halves lie more than 0.25 m apart along the branch axis."""
    l, w = box[3] * rng.uniform(0.8, 0.95), box[4] * rng.uniform(0.8, 0.95)
    k = int(0.7 * n)
    sx, sy = rng.choice([-1, 1]), rng.choice([-1, 1])
    long_side = np.stack([rng.uniform(-l / 2, l / 2, k), np.full(k, sy * w / 2)], 1)
    short_side = np.stack([np.full(n - k, sx * l / 2), rng.uniform(-w / 2, w / 2, n - k)], 1)
    xy = np.concatenate([long_side, short_side]) + rng.normal(0, 0.02, (n, 2)) + rng.uniform(-0.2, 0.2, 2)
    yaw = box[6] + rng.uniform(-0.15, 0.15)
    c, s = np.cos(yaw), np.sin(yaw)
    world = np.stack([xy[:, 0] * c - xy[:, 1] * s + box[0], xy[:, 0] * s + xy[:, 1] * c + box[1],
                      rng.uniform(0.3, 1.5, n)], 1)
    return world.astype(np.float32)[rng.permutation(n)]


def test_rotated_clusters_in_one_launch(G):
    rng = np.random.default_rng(12)
    segs = []
    for s in range(60):
        r, a = rng.uniform(5, 75), rng.uniform(-np.pi, np.pi)
        box = np.array([r * np.cos(a), r * np.sin(a), 0.9, rng.uniform(4.0, 5.2), rng.uniform(1.7, 2.1), 1.6,
                        rng.uniform(-np.pi, np.pi)])
        segs.append((car_cluster(rng, box, int(rng.integers(12, 900))), box, 0 if s % 15 != 7 else -1))
    got = orient_direct(G, segs)
    # 1e-4: one float32 entry of the device's cos / sin rounding the other way moves a centre by 2^-24 * 106 m = 1e-5 m, x 10
    worst = check_against_restatement(got, segs, exact_xy=False, tol=1e-4)
    assert np.mean(np.array(worst) <= 1e-9) >= 0.95, sorted(worst)[-5:]
    turned = [abs(got["box_orient"][s][6] - segs[s][1][6]) for s in range(60) if segs[s][2] >= 0]
    assert min(turned) > 0 and max(turned) > 0.05


def test_helpers_equal_the_batch_path(C, G):
    rng = np.random.default_rng(5)
    box = np.array([20.3, -7.1, 0.9, 4.7, 1.9, 1.6, 0.7])
    pts = car_cluster(rng, box, 200)
    got = orient_direct(G, [(pts, box, 0)])
    np.testing.assert_array_equal(C.correct_orientation(pts, box), got["box_orient"][0])
    np.testing.assert_array_equal(C.density_guided_drift(pts, box), got["box_drift"][0])
    np.testing.assert_array_equal(C.density_guided_drift(pts, C.correct_orientation(pts, box)), got["box_orient_drift"][0])
    full = np.concatenate([pts, np.ones((200, 2), np.float32)], 1)                # extra columns are ignored
    np.testing.assert_array_equal(C.density_guided_drift(full, box), got["box_drift"][0])


# ---- the golden sequence -----------------------------------------------------------------------------------------------------------

_RUN = {}


def resize_run(C, rz, chunk=16, sub_batch=128, again=False):
    """resize_frames over the golden input (the reference's _CSS infos and prototypes), once per (chunk, sub_batch)."""
    key = (chunk, sub_batch)
    if key not in _RUN or again:
        frames, css, proto = golden_inputs(rz)
        c = C.C_PROTO(str(rz["seq"]), "/nonexistent", CFG, chunk=chunk, sub_batch=sub_batch)
        c.resize_frames([f[:, 0:3] for f in frames], css, C.PrototypeTable(proto, PREDEFINED))
        if again:
            return css
        _RUN[key] = css
    return _RUN[key]


def test_golden_refine_box_size(C, rz):
    infos = resize_run(C, rz)
    check_resize(infos, rz, restated(rz)[1] if flagged(rz) else None)


def _same_infos(a, b):
    for x, y in zip(a, b):
        for k in ("outline_box", "outline_score", "outline_proto_id"):
            np.testing.assert_array_equal(x[k], y[k], err_msg=k)


@pytest.mark.parametrize("chunk,sub_batch", [(1, 128), (2, 128), (16, 2)])
def test_batching_gives_identical_output(C, rz, chunk, sub_batch):
    _same_infos(resize_run(C, rz), resize_run(C, rz, chunk, sub_batch))


def test_repetition_gives_identical_output(C, rz):
    _same_infos(resize_run(C, rz), resize_run(C, rz, again=True))


def test_driver_files_and_cache(C, rz, tmp_path, monkeypatch):
    frames, css, proto = golden_inputs(rz)
    seq = str(rz["seq"])
    os.makedirs(tmp_path / seq)
    for i, f in enumerate(frames):
        np.save(tmp_path / seq / ("%04d.npy" % i), f)
    for suffix, obj in (("_CSS", css), ("_CSS_proto", proto)):
        with open(tmp_path / seq / (seq + "_outline_MFCF" + suffix + ".pkl"), "wb") as f:
            pickle.dump(obj, f)
    c = C.C_PROTO(seq, str(tmp_path), CFG, chunk=2)
    resize = c.refine_box_size()
    _same_infos(resize, resize_run(C, rz))
    load = lambda suffix: pickle.load(open(tmp_path / seq / (seq + "_outline_C_PROTO" + suffix + ".pkl"), "rb"))
    _same_infos(load("_resize"), resize)
    final = c()                                    # stages one and two from their files, then refine_box_pos
    check_final(final, rz)
    check_final(load(""), rz)
    assert "outline_proto_id" in load("")[0]
    # the cached files return without constructing a CProtoGPU

    def no_gpu(*a, **k):
        raise AssertionError("the cached result must not launch anything")

    monkeypatch.setattr(C.cproto.CProtoGPU, "__init__", no_gpu)
    monkeypatch.setattr(C.RefineGPU, "run", no_gpu)
    again = C.C_PROTO(seq, str(tmp_path), CFG)
    _same_infos(again.refine_box_size(), resize)
    check_final(again.refine_box_pos(), rz)
    check_final(again(), rz)


def test_create_refined_from_the_initial_labels(C, tmp_path):
    """All four stages of a short synthetic sequence from its <seq>_outline_MFCF.pkl alone."""
    from cpd_amd.synthetic import cproto_sequence
    frames, infos = cproto_sequence(3, n_az=300)
    seq = "segment-00000042_short"
    os.makedirs(tmp_path / seq)
    for i, f in enumerate(frames):
        np.save(tmp_path / seq / ("%04d.npy" % i), f)
    with open(tmp_path / seq / (seq + "_outline_MFCF.pkl"), "wb") as f:
        pickle.dump(copy.deepcopy(infos), f)
    out = C.create_refined([seq], str(tmp_path), CFG, chunk=2)[0]
    for name in ("MFCF_CSS", "MFCF_CSS_raw_proto", "MFCF_CSS_proto", "C_PROTO_resize", "C_PROTO"):
        assert os.path.exists(tmp_path / seq / (seq + "_outline_" + name + ".pkl")), name
    saved = pickle.load(open(tmp_path / seq / (seq + "_outline_C_PROTO.pkl"), "rb"))
    assert len(saved) == len(frames) == len(out)
    for a, b, src in zip(saved, out, infos):
        _same_infos([a], [b])
        assert a["outline_proto_id"].dtype == np.longlong and a["outline_proto_id"].shape == src["outline_ids"].shape
        assert a["outline_box"].shape == src["outline_box"].shape
        skipped = src["outline_cls"] == "Dis_Small"
        assert (a["outline_proto_id"][skipped & (a["outline_cls"] == "Dis_Small")] == -1).all()
    assert any((a["outline_proto_id"] != -1).any() for a in saved)
