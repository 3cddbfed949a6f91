"""GPU checks of the MFCF generator (cpd_amd.mfcf, csrc/mfcf.hip) against the numpy restatement (tests/ref_mfcf.py) and the
reference's golden (tests/golden/mfcf.npz): the aggregation, voxel_sampling, box_fit_DGD's corrections, the per-frame chain, the
written file and the one-call forms."""
import copy
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_golden_mfcf as MG  # noqa: E402
import ref_mfcf as RM  # noqa: E402

pytestmark = pytest.mark.gpu

E2E_FRAMES = 6      # the written-file tests run the restatement on the host: a shorter drive keeps them to seconds


@pytest.fixture(scope="module")
def M():
    from cpd_amd import mfcf
    return mfcf


@pytest.fixture(scope="module")
def gpu(M):
    return M.MFCFGPU(MG.golden_config()["GeneratorConfig"])


@pytest.fixture(scope="module")
def gold():
    z = dict(np.load(os.path.join(HERE, "golden", "mfcf.npz")))
    frames, poses = MG.sequence(int(z["seed"]), int(z["n_frames"]), int(z["n_az"]))
    assert MG.digest(frames, poses) == str(z["digest"])
    return z, frames, poses, [z["h%d" % i] for i in range(len(frames))]


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---- gather ------------------------------------------------------------------------------------------------------------------------

def test_gather_is_the_restatement_bit_for_bit(M, gpu):
    import torch
    rng = np.random.default_rng(11)
    t = np.float16(0.7)
    edge = np.array([np.nextafter(t, np.float16(0)), t, np.nextafter(t, np.float16(1)), np.nan], np.float16)
    frames, scores, poses = [], [], []
    for k, (n, dt) in enumerate([(301, np.float16), (297, np.float32), (310, np.float16)]):
        frames.append(np.concatenate([rng.uniform(-40, 40, (n, 2)), rng.uniform(-2, 3, (n, 3))], 1).astype(dt))
        h = rng.uniform(0.4, 1.0, n).astype(np.float16)
        h[:8] = np.tile(edge, 2)
        scores.append(h)
        a = 0.3 * k + 0.1
        pose = np.eye(4)
        pose[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        pose[:3, 3] = [5321.7 + 3.1 * k, -2811.3 + 0.7 * k, 41.2]
        poses.append(pose)
    assert ((scores[0] > 0.7) != (scores[0].astype(np.float64) > 0.7)).any()     # the float16 threshold is not the float64 one
    # frame 0: negative j are skipped; frame 2 with sweep 1 missing; frame 1 with everything
    wins = [M.window(0, 2, 1, lambda j: j < 3), M.window(2, 2, 1, lambda j: j in (0, 2)), M.window(1, 2, 1, lambda j: j < 3)]
    cur = [0, 2, 1]
    assert wins == [[0, 1], [0, 2], [0, 1, 2]]
    sweeps = [gpu.upload(f, h) for f, h in zip(frames, scores)]
    rows, off, count, off_host = gpu.gather(sweeps, poses, wins, cur, 0.7)
    torch.cuda.synchronize()
    rows, count = rows.cpu().numpy(), count.cpu().numpy()
    for f, (w, c) in enumerate(zip(wins, cur)):
        want = RM.gather(frames, scores, poses, c, w, 0.7)
        assert count[f] == len(want) < off_host[f + 1] - off_host[f]
        _bits_equal(rows[off_host[f]:off_host[f] + count[f]], want)


# ---- voxel_sampling ----------------------------------------------------------------------------------------------------------------

def _voxel(gpu, slices, caps=None):
    """The kernel over slices (float32 [n, 3] each) laid out with room to spare: per slice the sampled rows."""
    import torch
    caps = caps or [len(s) + 7 for s in slices]
    off = np.zeros(len(slices) + 1, np.int32)
    off[1:] = np.cumsum(caps)
    buf = np.full((max(int(off[-1]), 1), 3), np.nan, np.float32)      # the room between slices must never be read
    for s, o in zip(slices, off):
        buf[o:o + len(s)] = s
    dev = gpu.device
    out, src, out_off, err = gpu.voxel_sample(torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev),
                                              torch.tensor([len(s) for s in slices], dtype=torch.int32, device=dev), len(slices))
    out, src, out_off = out.cpu().numpy(), src.cpu().numpy(), out_off.cpu().numpy()
    assert int(err.item()) == 0
    assert out_off[0] == 0 and out_off[-1] == off[-1] and (np.diff(out_off) >= 0).all()
    assert not out[out_off[-2]:].any()                               # the tail is one more, all-zero frame
    res = [out[out_off[f]:out_off[f + 1]] for f in range(len(slices))]
    for f, s in enumerate(slices):
        _bits_equal(s[src[out_off[f]:out_off[f + 1]]], res[f])
    return res


def test_voxel_sampling_hand_built_slice(gpu):
    r = np.float32(0.1)
    b3, b7 = np.float32(3) * r, np.float32(7) * r
    xs = [0.05, 0.0, 0.06, b3, np.nextafter(b3, np.float32(1)), np.nextafter(b3, np.float32(0)), 0.07,
          b7, np.nextafter(b7, np.float32(1)), np.nextafter(b7, np.float32(0)), 2.0]
    pts = np.zeros((len(xs), 3), np.float32)
    pts[:, 0] = xs
    pts[:, 1] = np.arange(len(xs)) * 1e-3          # tells the rows of one cell apart
    got = _voxel(gpu, [pts])[0]
    cells = {}
    for p in pts:                                  # the reference's loop: a dict keyed by cell, values overwritten
        cells[tuple(((p - pts.min(0)) // 0.1).tolist())] = p
    want = np.array(list(cells.values()))
    _bits_equal(got, want)
    _bits_equal(got, RM.voxel_sampling(pts))
    # rows 0, 1, 2 and 6 share the first cell: the last of them (0.07) comes out, at the first one's place
    assert got[0, 0] == np.float32(0.07) and len(got) < len(pts)


def test_voxel_sampling_colliding_rows_and_several_frames(gpu):
    rng = np.random.default_rng(12)
    cube = rng.uniform(0, 1, (1025, 3)).astype(np.float32)            # 1000 cells: most rows collide, more than one workgroup
    wide = rng.uniform(-30, 30, (333, 3)).astype(np.float32)
    got = _voxel(gpu, [cube, np.zeros((0, 3), np.float32), wide, cube[:64]], caps=[1025, 0, 340, 64])
    assert len(got[0]) < 700 and len(got[1]) == 0
    for g, s in zip(got, [cube, None, wide, cube[:64]]):
        if s is not None:
            _bits_equal(g, RM.voxel_sampling(s))


# ---- box_fit_DGD -------------------------------------------------------------------------------------------------------------------

def _l_cluster(rng, yaw, centre, dense_x=1, dense_y=1, tall_x=1, n=260):
    """An L-shaped cluster as a scan sees a vehicle: a long side and a short side meeting at one corner, the corner chosen by
    dense_x / dense_y, the taller end by tall_x; float32 rows in world coordinates, ground-level rows included."""
    l, w = rng.uniform(3.6, 5.0), rng.uniform(1.6, 2.1)
    a = np.stack([rng.uniform(-l / 2, l / 2, n), np.full(n, dense_y * w / 2) + rng.normal(0, 0.02, n)], 1)
    b = np.stack([np.full(n // 2, dense_x * l / 2) + rng.normal(0, 0.02, n // 2), rng.uniform(-w / 2, w / 2, n // 2)], 1)
    xy = np.concatenate([a, b])
    height = np.where(xy[:, 0] * tall_x > 0, 1.7, 1.1)
    z = rng.uniform(0, 1, len(xy)) * height
    c, s = np.cos(yaw), np.sin(yaw)
    world = np.stack([xy[:, 0] * c - xy[:, 1] * s + centre[0], xy[:, 0] * s + xy[:, 1] * c + centre[1], z], 1)
    return world.astype(np.float32).astype(np.float64)


def _fitter(M, **kw):
    return M.OutlineFitter(**dict(dict(ground_min_threshold=[0.2, -0.5, -0.5], cluster_min_points=5, min_box_volume=0.1,
                                       min_box_height=0.3), **kw))


def _fit_cfg(**kw):
    return dict(dict(MG.golden_config()["GeneratorConfig"]), **kw)


def test_dgd_rotated_clusters_take_every_branch(M):
    rng = np.random.default_rng(13)
    clusters = [_l_cluster(rng, rng.uniform(-np.pi, np.pi), rng.uniform(-30, 30, 2), rng.choice([-1, 1]), rng.choice([-1, 1]),
                           rng.choice([-1, 1])) for _ in range(60)]
    got, bits = _fitter(M).box_fit_DGD(clusters, return_bits=True)
    want, want_bits = RM.box_fit_dgd(clusters, _fit_cfg(), return_bits=True)
    assert len(want) == 60
    np.testing.assert_array_equal(bits, want_bits)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    for bit in (M.BIT_DRIFT_X, M.BIT_DRIFT_Y, M.BIT_ORIENT_MAX, M.BIT_FLIPPED):       # both sides of each, in one launch
        assert 3 <= int(((bits & bit) != 0).sum()) <= 57, bit
    assert ((bits & M.BIT_ORIENT_X) != 0).all() and ((bits & M.BIT_TURNED) != 0).all()


@pytest.mark.parametrize("dense_x,dense_y,tall_x", [(1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1)])
def test_dgd_one_branch_at_a_time(M, dense_x, dense_y, tall_x):
    """One L per corner: the three steps one by one through the one-call kernel path against the restatement's steps."""
    import ref_cproto_refine as RR
    rng = np.random.default_rng(14)
    pts = _l_cluster(rng, 0.4, (12.0, -7.0), dense_x, dense_y, tall_x)
    pts = pts[pts[:, 2] > pts[:, 2].min() + 0.2]
    box0 = np.asarray(_fitter(M).box_fit([pts]))[0]
    g = M._gpu()
    b1, bits1 = M._dgd_one(g, [pts], box0, M.STEP_DRIFT | M.STEP_ALL_ROWS)
    np.testing.assert_allclose(b1[0], RR.density_guided_drift(pts, box0), rtol=0, atol=1e-9)
    info = {}
    want2 = RR.correct_orientation(pts, b1[0], info=info)
    b2, bits2 = M._dgd_one(g, [pts], b1[0], M.STEP_ORIENT | M.STEP_ALL_ROWS)
    np.testing.assert_allclose(b2[0], want2, rtol=0, atol=1e-9)
    assert bool(bits2[0] & M.BIT_ORIENT_MAX) == (info["side"] == 'max') and bool(bits2[0] & M.BIT_ORIENT_X) == (info["branch"] == 'x')
    head = {}
    want3 = RM.correct_heading(pts, b2[0], head)
    b3, bits3 = M._dgd_one(g, [pts], b2[0], M.STEP_HEADING | M.STEP_ALL_ROWS)
    np.testing.assert_allclose(b3[0], want3, rtol=0, atol=1e-9)
    assert bool(bits3[0] & M.BIT_FLIPPED) == head["flipped"]
    # the whole of box_fit_DGD's tail is the three in this order (not orientation first)
    ball, bits = M._dgd_one(g, [pts], box0, 7 | M.STEP_ALL_ROWS)
    np.testing.assert_allclose(ball[0], want3, rtol=0, atol=1e-9)
    assert bits[0] == (bits1[0] | bits2[0] | bits3[0]) == RM.dgd(pts, box0)[1]


def test_dgd_orientation_along_y_and_empty_slabs(M):
    """Branches box_fit_DGD's own boxes never reach: a box much longer than its cluster (orientation bins along y), slabs without
    rows, and a cluster that lies in one half of the box (an empty list of maxima counts as 0)."""
    rng = np.random.default_rng(15)
    g = M._gpu()
    wedge = np.stack([rng.uniform(-0.8, 0.8, 300), rng.uniform(-1.0, 1.0, 300), rng.uniform(0.3, 1.5, 300)], 1)
    wedge[:, 0] += 0.25 * wedge[:, 1]
    wedge = wedge.astype(np.float32).astype(np.float64)
    box = np.array([0.1, 0.05, 0.8, 9.0, 2.0, 1.6, 0.2])
    info = {}
    want = RM.dgd(wedge, box)
    RM.RR.correct_orientation(wedge, RM.RR.density_guided_drift(wedge, box), info=info)
    assert info["branch"] == 'y'
    got, bits = M._dgd_one(g, [wedge], box, 7 | M.STEP_ALL_ROWS)
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-9)
    assert bits[0] == want[1] and not bits[0] & M.BIT_ORIENT_X
    # two blobs at the ends of a long box: slabs 2..7 hold no row
    ends = np.concatenate([wedge * [0.3, 0.5, 1.0] + [-3.0, 0, 0], wedge * [0.3, 0.5, 0.6] + [3.0, 0, 0]])
    ends = ends.astype(np.float32).astype(np.float64)
    long_box = np.array([[0.0, 0.0, 0.8, 8.0, 2.0, 1.6, 0.0]])
    head = {}
    want = RM.correct_heading(ends, long_box[0], head)
    assert head["n_min"] < 5 and head["flipped"] is False
    assert M.correct_heading(ends, long_box) is long_box
    turned = M.correct_heading(ends * [-1.0, 1.0, 1.0], long_box)
    assert turned is not long_box and turned[0, 6] == RM.correct_heading(ends * [-1.0, 1.0, 1.0], long_box[0])[6]
    # every row in the front half: the rear list is empty and counts as 0, below the front's mean
    front = wedge * [0.3, 0.5, 1.0] + [2.0, 0, 0.9]
    front = front.astype(np.float32).astype(np.float64)
    head = {}
    want = RM.correct_heading(front, long_box[0], head)
    assert head["n_min"] == 1 and head["flipped"] is True        # the list of one 0 the reference appends
    np.testing.assert_allclose(M.correct_heading(front, long_box)[0], want, rtol=0, atol=1e-9)


def test_dgd_more_boxes_than_the_old_segment_limit(M):
    rng = np.random.default_rng(16)
    n_boxes = 1100                                                   # cpd_refine_orient_drift stops at 1022 segments
    base = np.concatenate([rng.uniform([-0.6, -0.3, 0.0], [0.6, 0.3, 0.0], (4, 3)),
                           rng.uniform([-0.6, -0.3, 0.4], [0.6, 0.3, 1.2], (8, 3))])
    clusters = []
    for k in range(n_boxes):
        a = 0.01 * k
        rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        c = base @ rot.T + [4.0 * (k % 40) - 80, 4.0 * (k // 40) - 55, 0]
        clusters.append(c.astype(np.float32).astype(np.float64))
    got, bits = _fitter(M, min_box_volume=0.01).box_fit_DGD(clusters, return_bits=True)
    want, want_bits = RM.box_fit_dgd(clusters, _fit_cfg(min_box_volume=0.01), return_bits=True)
    assert len(want) == n_boxes
    np.testing.assert_array_equal(bits, want_bits)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


# ---- the per-frame chain and the written file --------------------------------------------------------------------------------------

def test_per_frame_chain_on_the_golden_sequence(M, gold, tmp_path):
    z, frames, poses, scores = gold
    MG.write_sequence(str(tmp_path), frames, poses, scores)
    infos = [dict(pose=p) for p in poses]
    gen = M.MFCF(MG.SEQ, str(tmp_path), MG.golden_config(), chunk=5)      # three chunks, the last one short
    boxes, got_poses, bits, vox = gen.per_frame_boxes(infos, stages=True)
    n_box = n_flag = 0
    for i in range(len(frames)):
        assert len(vox[i]) == int(z["vox%d_n" % i]) and MG.rows_digest(vox[i]) == str(z["vox%d_digest" % i]), "frame %d" % i
        ref, flag = z["pf%d_box" % i], z["pf%d_flag" % i]
        b = np.asarray(boxes[i], np.float64).reshape(-1, 7)
        assert b.shape == ref.shape
        np.testing.assert_allclose(b[~flag], ref[~flag], rtol=0, atol=1e-9)
        np.testing.assert_array_equal(bits[i][~flag], z["pf%d_bits" % i][~flag])
        n_box, n_flag = n_box + len(ref), n_flag + int(flag.sum())
    assert n_box >= 40 and n_flag <= 0.10 * n_box


@pytest.fixture(scope="module")
def short_drive(gold):
    """The first E2E_FRAMES frames as a sequence of their own, with the restatement's per-frame boxes (computed once)."""
    z, frames, poses, scores = gold
    frames, poses, scores = frames[:E2E_FRAMES], poses[:E2E_FRAMES], scores[:E2E_FRAMES]
    cfg = MG.golden_config()
    per_frame = RM.sequence_boxes(frames, scores, poses, cfg["GeneratorConfig"])
    return frames, poses, scores, cfg, per_frame


def _tracked(per_frame, poses, cfg):
    from cpd_amd.tracker import TrackSmooth
    ts = TrackSmooth(cfg["GeneratorConfig"])
    ts.tracking([copy.deepcopy(b) for b in per_frame], [p.copy() for p in poses])
    return [ts.get_current_frame_objects_and_cls(i) for i in range(len(poses))]


def _check_infos(infos, want, atol=1e-6):
    assert len(infos) == len(want)
    for info, (b, ids, cls, dif) in zip(infos, want):
        assert set(info) >= {'pose', 'outline_box', 'outline_ids', 'outline_cls', 'outline_dif'}
        assert info['outline_box'].shape == b.shape and info['outline_box'].shape[1] == 7
        np.testing.assert_array_equal(info['outline_ids'], ids)
        np.testing.assert_array_equal(info['outline_cls'], cls)
        np.testing.assert_array_equal(info['outline_dif'], dif)
        np.testing.assert_allclose(info['outline_box'], b, rtol=0, atol=atol)


def test_written_file_end_to_end(M, short_drive, tmp_path, monkeypatch):
    frames, poses, scores, cfg, per_frame = short_drive
    root = str(tmp_path)
    MG.write_sequence(root, frames, poses, scores)
    out_pkl = os.path.join(root, MG.SEQ, MG.SEQ + "_outline_MFCF.pkl")
    infos = M.MFCF(MG.SEQ, root, cfg)()
    want = _tracked(per_frame, poses, cfg)
    assert sum(len(w[0]) for w in want) >= 40
    _check_infos(infos, want)
    with open(out_pkl, "rb") as f:
        _check_infos(pickle.load(f), want)
    # the second call answers from the file: no kernel, no frame is touched
    monkeypatch.setattr(M.MFCFGPU, "frames_boxes", lambda *a, **k: pytest.fail("the cached file must be returned as it is"))
    again = M.MFCF(MG.SEQ, root, cfg)()
    _check_infos(again, want)
    # the refiner chain starts from the written file
    from cpd_amd import cproto_refine
    rcfg = copy.deepcopy(cproto_refine.REFINE_CONFIG)
    rcfg["GeneratorConfig"] = cfg["GeneratorConfig"]
    refined = cproto_refine.create_refined([MG.SEQ], root, rcfg)[0]
    assert len(refined) == len(frames) and all('outline_score' in r for r in refined)


def _tainted_tracks(z, poses, cfg):
    """The ids of the tracks that take a flagged per-frame box (one where the restatement leaves the reference by more than
    1e-9): the golden's per-frame boxes through the tracker, detection by detection."""
    from cpd_amd.tracker import Tracker3D
    trk = Tracker3D(box_type='OpenPCDet', config=cfg["GeneratorConfig"])
    tainted = set()
    for i, pose in enumerate(poses):
        boxes = MG.frame_boxes(z, i)
        _, ids = trk.tracking(boxes, scores=np.ones(len(boxes)) * 100, pose=pose.copy(), timestamp=i)
        assert len(ids) == len(boxes)
        tainted |= set(np.asarray(ids)[z["pf%d_flag" % i]].tolist())
    return tainted


def test_written_file_against_the_references_final_infos(M, gold, tmp_path):
    """All twelve frames: the written ids are the reference's; on every track that takes no flagged box the classes are too
    and the boxes agree to 1e-6."""
    z, frames, poses, scores = gold
    cfg = MG.golden_config()
    MG.write_sequence(str(tmp_path), frames, poses, scores)
    infos = M.MFCF(MG.SEQ, str(tmp_path), cfg)()
    tainted = _tainted_tracks(z, poses, cfg)
    n_clean = 0
    for info, want in zip(infos, MG.unpack_infos(z, "fin", poses)):
        np.testing.assert_array_equal(info['outline_ids'], want['outline_ids'])
        np.testing.assert_array_equal(info['outline_dif'], want['outline_dif'])
        clean = ~np.isin(want['outline_ids'], sorted(tainted))
        np.testing.assert_array_equal(info['outline_cls'][clean], want['outline_cls'][clean])
        np.testing.assert_allclose(info['outline_box'][clean], want['outline_box'][clean], rtol=0, atol=1e-6)
        n_clean += int(clean.sum())
    assert n_clean >= 150 and len(tainted) >= 1


def test_create_mfcf_equals_single_runs(M, gold, short_drive, tmp_path):
    z, all_frames, all_poses, all_scores = gold
    frames, poses, scores, cfg, _ = short_drive
    second = "segment-87654322_mfcf"
    sl = slice(E2E_FRAMES, 2 * E2E_FRAMES)
    for root in (str(tmp_path / "a"), str(tmp_path / "b")):
        MG.write_sequence(root, frames, poses, scores)
        MG.write_sequence(root, all_frames[sl], all_poses[sl], all_scores[sl], seq=second)
    both = M.create_mfcf([MG.SEQ, second], str(tmp_path / "a"), cfg, chunk=4)
    singles = [M.MFCF(s, str(tmp_path / "b"), cfg)() for s in (MG.SEQ, second)]
    for got, want in zip(both, singles):
        assert len(got) == len(want) == E2E_FRAMES
        for g, w in zip(got, want):
            for k in ('outline_box', 'outline_ids', 'outline_cls', 'outline_dif'):
                np.testing.assert_array_equal(g[k], w[k])


# ---- one call each -----------------------------------------------------------------------------------------------------------------

def test_one_call_forms(M):
    rng = np.random.default_rng(17)
    pts = np.concatenate([rng.uniform(-3, 3, (500, 3)), rng.uniform(0, 1, (500, 2))], 1).astype(np.float32)
    got = M.voxel_sampling(pts)
    want, idx = RM.voxel_sampling(np.ascontiguousarray(pts[:, :3]), return_index=True)
    assert got.shape[1] == 5 and got.dtype == np.float32
    _bits_equal(got, pts[idx])
    cluster = _l_cluster(rng, -1.1, (-8.0, 15.0), -1, 1, 1)
    boxes = _fitter(M).box_fit_DGD([cluster])
    want = RM.box_fit_dgd([cluster], _fit_cfg())
    assert np.asarray(boxes).shape == (1, 7)
    np.testing.assert_allclose(boxes, want, rtol=0, atol=1e-9)
    assert _fitter(M).box_fit_DGD([]) == []
    box = np.asarray(boxes)
    kept = cluster[cluster[:, 2] > cluster[:, 2].min() + 0.2]
    out = M.correct_heading(kept, box)
    np.testing.assert_allclose(out[0], RM.correct_heading(kept, box[0]), rtol=0, atol=1e-9)
