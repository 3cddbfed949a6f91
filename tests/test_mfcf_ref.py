"""CPU checks of the MFCF generator (cpd_amd.mfcf, cpd_amd.tracker): the numpy restatement (tests/ref_mfcf.py) against the
reference's golden (tests/golden/mfcf.npz, made by make_golden_mfcf.py), the host tracker against the golden final infos, the
floor_divide restatement against numpy, the argument checks, the dispatcher, the caching and the config -- no GPU anywhere."""
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

FLAG_CAP = 0.10


@pytest.fixture(scope="module")
def gold():
    z = dict(np.load(os.path.join(HERE, "golden", "mfcf.npz")))
    frames, poses = MG.sequence(int(z["seed"]), int(z["n_frames"]), int(z["n_az"]))
    assert MG.digest(frames, poses) == str(z["digest"]), "synthetic.ppscore_sequence no longer gives the golden's input"
    scores = [z["h%d" % i] for i in range(len(frames))]
    return z, frames, poses, scores


@pytest.fixture(scope="module")
def restated(gold):
    """The restatement's per-frame stages, computed once."""
    z, frames, poses, scores = gold
    return RM.sequence_boxes(frames, scores, poses, MG.golden_config()["GeneratorConfig"], stages=True)


def test_restatement_voxel_sampling_is_the_references(gold, restated):
    z = gold[0]
    for i, (_, _, vox) in enumerate(restated):
        assert len(vox) == int(z["vox%d_n" % i])
        assert MG.rows_digest(vox) == str(z["vox%d_digest" % i]), "frame %d" % i


def test_restatement_boxes_are_the_references(gold, restated):
    z = gold[0]
    n_box = n_flag = 0
    for i, (boxes, bits, _) in enumerate(restated):
        ref, flag = z["pf%d_box" % i], z["pf%d_flag" % i]
        boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
        assert boxes.shape == ref.shape
        np.testing.assert_array_equal(np.asarray(bits, np.int32), z["pf%d_bits" % i])
        if (~flag).any():
            np.testing.assert_allclose(boxes[~flag], ref[~flag], rtol=0, atol=1e-9)
        n_box += len(ref)
        n_flag += int(flag.sum())
    assert n_box >= 40
    assert n_flag <= FLAG_CAP * n_box


def _same_infos(got, want, atol):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.asarray(g['outline_box']).shape == w['outline_box'].shape, "frame %d" % i
        assert np.asarray(g['outline_box']).shape[1:] == (7,)
        for k in ('outline_ids', 'outline_cls', 'outline_dif'):
            assert np.asarray(g[k]).shape == w[k].shape, "frame %d %s" % (i, k)
        if len(w['outline_box']) == 0:
            continue
        np.testing.assert_array_equal(g['outline_ids'], w['outline_ids'])
        np.testing.assert_array_equal(g['outline_cls'], w['outline_cls'])
        np.testing.assert_array_equal(g['outline_dif'], w['outline_dif'])
        np.testing.assert_allclose(g['outline_box'], w['outline_box'], rtol=0, atol=atol)


def _track(gold, cfg):
    from cpd_amd.tracker import TrackSmooth
    z, _, poses, _ = gold
    ts = TrackSmooth(cfg)
    ts.tracking([MG.frame_boxes(z, i) for i in range(len(poses))], [p.copy() for p in poses])
    infos = []
    for i in range(len(poses)):
        b, ids, cls, dif = ts.get_current_frame_objects_and_cls(i)
        infos.append(dict(outline_box=b, outline_ids=ids, outline_cls=cls, outline_dif=dif))
    return ts, infos


def test_tracker_reproduces_the_golden_final_infos(gold):
    z, _, poses, _ = gold
    ts, infos = _track(gold, MG.golden_config()["GeneratorConfig"])
    _same_infos(infos, MG.unpack_infos(z, "fin", poses), 1e-9)
    counts = dict(zip(z["counts_keys"].tolist(), z["counts_vals"].tolist()))
    assert counts["died_missed"] >= 1 and counts["died_new"] >= 1 and counts["interpolated"] >= 1
    dead = ts.tracker.dead_trajectories.values()
    assert sum(1 for t in dead if t.consecutive_missed_num >= MG.MAX_PREDICTION_NUM) == counts["died_missed"]
    assert sum(1 for t in dead if len(t) - t.consecutive_missed_num == 1
               and t.consecutive_missed_num < MG.MAX_PREDICTION_NUM) == counts["died_new"]
    assert len(ts.tracker.dead_trajectories) + len(ts.tracker.active_trajectories) == counts["tracks"]


def test_tracker_with_size_and_yaw_smoothing(gold):
    """lwh_win_size = yaw_win_size = 3: the distance softmax and the yaw residual mean (the yaml's 0 switches them off)."""
    z, _, poses, _ = gold
    _, infos = _track(gold, MG.golden_config(smooth=True)["GeneratorConfig"])
    _same_infos(infos, MG.unpack_infos(z, "smo", poses), 1e-9)


def test_tracker_turns_boxes_with_l_below_w(gold):
    """box_fit never hands out l < w, so the golden's third pass exchanges them in every third box: filtering swaps them back and
    adds pi / 2 to the heading."""
    from cpd_amd.tracker import TrackSmooth
    z, _, poses, _ = gold
    counts = dict(zip(z["counts_keys"].tolist(), z["counts_vals"].tolist()))
    assert counts["swaps"] >= 3
    ts = TrackSmooth(MG.golden_config(smooth=True)["GeneratorConfig"])
    ts.tracking(MG.swapped_boxes([MG.frame_boxes(z, i) for i in range(len(poses))]), [p.copy() for p in poses])
    infos = []
    for i in range(len(poses)):
        b, ids, cls, dif = ts.get_current_frame_objects_and_cls(i)
        infos.append(dict(outline_box=b, outline_ids=ids, outline_cls=cls, outline_dif=dif))
    _same_infos(infos, MG.unpack_infos(z, "swp", poses), 1e-9)


def test_tracker_takes_attribute_configs_and_number_classes(gold):
    import types
    from cpd_amd.tracker import TrackSmooth
    z, _, poses, _ = gold
    cfg = MG.golden_config()["GeneratorConfig"]
    ts = TrackSmooth(types.SimpleNamespace(**cfg))
    ts.tracking([MG.frame_boxes(z, i) for i in range(len(poses))], [p.copy() for p in poses])
    i = next(i for i in range(len(poses)) if len(z["fin%d_box" % i]))
    _, _, names, _ = ts.get_current_frame_objects_and_cls(i)
    _, _, numbers, _ = ts.get_current_frame_objects_and_cls(i, return_name=False)
    assert [cfg["cls"][n] for n in names] == numbers.tolist()
    empty = ts.get_current_frame_objects_and_cls(len(poses) + 5)
    assert [e.shape for e in empty] == [(0, 7), (0,), (0,), (0,)]


def test_tracker_details():
    from cpd_amd import tracker as T
    # register_bbs rewrites its input in place; convert_bbs_type hands out a copy
    pose = np.eye(4)
    pose[:3, 3] = [10.0, -5.0, 1.0]
    boxes = np.array([[1.0, 2.0, 0.5, 4.0, 2.0, 1.5, 0.3]])
    same = T.register_bbs(boxes, pose)
    assert same is boxes and boxes[0, 0] == 11.0 and boxes[0, 1] == -3.0
    assert T.convert_bbs_type(boxes, "OpenPCDet") is not boxes
    with pytest.raises(NotImplementedError, match="Kitti"):
        T.convert_bbs_type(boxes, "Kitti")
    online = dict(MG.golden_config()["GeneratorConfig"], latency=0.5)
    ts = T.TrackSmooth(online)
    with pytest.raises(NotImplementedError, match="latency"):
        ts.tracking([boxes.copy()], [np.eye(4)])
    # an empty frame arrives as []; greedy association blanks the taken column
    cfg = MG.golden_config()["GeneratorConfig"]
    trk = T.Tracker3D(box_type='OpenPCDet', config=cfg)
    b, ids = trk.tracking([], scores=np.zeros(0), pose=np.eye(4), timestamp=0)
    assert b.shape == (0, 7) and ids.shape == (0,)
    two = np.array([[0.0, 0.0, 0.5, 4.0, 2.0, 1.5, 0.0], [0.2, 0.0, 0.5, 4.0, 2.0, 1.5, 0.0]])
    _, ids0 = trk.tracking(two[:1].copy(), scores=np.ones(1) * 100, pose=np.eye(4), timestamp=1)
    _, ids1 = trk.tracking(two.copy(), scores=np.ones(2) * 100, pose=np.eye(4), timestamp=2)
    assert ids0.tolist() == [0] and ids1.tolist() == [0, 1]      # the second detection may not take track 0 again
    # the second object of a track takes its velocity from the two detections
    st = trk.active_trajectories[0].trajectory[2].updated_state
    assert st.shape == (13, 1) and st[3, 0] == pytest.approx(0.0)
    _, ids2 = trk.tracking(np.array([[50.0, 0.0, 0.5, 4.0, 2.0, 1.5, 0.0]]), scores=np.ones(1) * 100, pose=np.eye(4), timestamp=3)
    assert ids2.tolist() == [2]
    assert len(trk.active_trajectories[1]) == 2 and trk.active_trajectories[1].consecutive_missed_num == 1


def test_floor_divide_restatement_is_numpys():
    rng = np.random.default_rng(5)
    res = np.float32(0.1)
    k = rng.integers(0, 3000, 4000).astype(np.float32)
    bound = (k * res).astype(np.float32)
    a = np.concatenate([bound, np.nextafter(bound, np.float32(np.inf)), np.nextafter(bound, np.float32(-np.inf)),
                        rng.uniform(0, 300, 4000).astype(np.float32), np.zeros(1, np.float32)])
    a = a[a >= 0]
    want = np.floor_divide(a, res)
    assert want.dtype == np.float32
    np.testing.assert_array_equal(RM.floor_divide32(a, res), want)
    assert (want != np.floor(a / res)).any(), "the cases must include rows where floor(a / b) is not floor_divide(a, b)"
    # a float32 scalar against the Python float 0.1, as voxel_sampling meets it
    for v in a[:200]:
        assert (v // 0.1) == RM.floor_divide32(np.array([v]), 0.1)[0]


def test_voxel_sampling_restatement_is_a_dict_of_cells():
    rng = np.random.default_rng(6)
    pts = rng.uniform(-1, 1, (700, 3)).astype(np.float32)
    pts[5] = pts[0]
    pts[9, :] = pts[0] + np.float32(1e-4)
    cells = {}
    mins = pts.min(0)
    for p in pts:
        cells[tuple(((p - mins) // 0.1).tolist())] = p
    want = np.array(list(cells.values()))
    got, idx = RM.voxel_sampling(pts, return_index=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(pts[idx], got)


def test_threshold_is_numpys_float16_comparison():
    from cpd_amd.mfcf import threshold_f16
    t = np.float16(0.7)
    h = np.array([np.nextafter(t, np.float16(0)), t, np.nextafter(t, np.float16(1)), np.nan], np.float16)
    want = h > 0.7
    assert want.tolist() == [False, False, True, False]
    np.testing.assert_array_equal(h.astype(np.float32) > np.float32(threshold_f16(0.7)), want)


def test_argument_checks():
    from cpd_amd import mfcf as M
    with pytest.raises(ValueError, match="multiple of frame_interval"):
        M.window(3, 5, 2, lambda j: True)
    with pytest.raises(NotImplementedError, match="at most 16 sweeps"):
        M.window(20, 10, 1, lambda j: True)
    assert M.window(2, 5, 1, lambda j: j != 4 and j < 6) == [0, 1, 2, 3, 5]      # negative j, a missing file
    assert len(M.window(20, 8, 1, lambda j: True)) == 16
    with pytest.raises(ValueError, match="PP scores for a frame"):
        M._check_scores(np.zeros(9, np.float16), 10)
    with pytest.raises(TypeError, match="float16"):
        M._check_scores(np.zeros(10, np.float32), 10)
    with pytest.raises(TypeError, match="float16 or float32"):
        M._check_points(np.zeros((4, 3), np.float64))
    with pytest.raises(ValueError):
        M._check_points(np.zeros((4, 2), np.float32))
    with pytest.raises(TypeError, match="float32 rows"):
        M.voxel_sampling(np.zeros((4, 3), np.float16))
    with pytest.raises(ValueError, match="chunk"):
        M.MFCF("s", "/nonexistent", M.MFCF_CONFIG, chunk=0)


def test_generator_checks_its_config_before_reading_frames(tmp_path):
    from cpd_amd import mfcf as M
    seq = "segment-00000001_x"
    MG.write_sequence(str(tmp_path), [np.zeros((4, 5), np.float32)] * 2, [np.eye(4)] * 2, seq=seq)
    cfg = copy.deepcopy(M.MFCF_CONFIG)
    cfg["GeneratorConfig"].update(frame_num=5, frame_interval=2)
    with pytest.raises(ValueError, match="multiple of frame_interval"):
        M.MFCF(seq, str(tmp_path), cfg)()
    cfg["GeneratorConfig"].update(frame_num=20, frame_interval=1)
    MG.write_sequence(str(tmp_path), [np.zeros((4, 5), np.float32)] * 40, [np.eye(4)] * 40, seq=seq)
    with pytest.raises(NotImplementedError, match="at most 16 sweeps"):
        M.MFCF(seq, str(tmp_path), cfg)()
    assert not os.path.exists(os.path.join(str(tmp_path), seq, seq + "_outline_MFCF.pkl"))


def test_cached_output_is_returned_as_it_is(tmp_path):
    from cpd_amd import mfcf as M
    seq = "segment-00000002_x"
    os.makedirs(os.path.join(str(tmp_path), seq))
    marker = [dict(pose=np.eye(4), outline_box=np.zeros((1, 7)), marker="cached")]
    with open(os.path.join(str(tmp_path), seq, seq + "_outline_MFCF.pkl"), "wb") as f:
        pickle.dump(marker, f)
    got = M.MFCF(seq, str(tmp_path), M.MFCF_CONFIG)()           # no input pkl, no frames, no GPU: the cache answers
    assert got[0]["marker"] == "cached"
    assert M.create_mfcf([seq], str(tmp_path), M.MFCF_CONFIG)[0][0]["marker"] == "cached"
    assert M.compute_outline_box(seq, str(tmp_path), M.MFCF_CONFIG)[0]["marker"] == "cached"


def test_dispatcher(tmp_path):
    from cpd_amd import mfcf as M
    from cpd_amd import outline as O
    seq = "segment-00000003_x"
    os.makedirs(os.path.join(str(tmp_path), seq))
    for name in ("DBSCAN", "MFCF"):
        with open(os.path.join(str(tmp_path), seq, "%s_outline_%s.pkl" % (seq, name)), "wb") as f:
            pickle.dump([dict(marker=name)], f)
    assert M.compute_outline_box(seq, str(tmp_path), dict(InitLabelGenerator="DBSCAN",
                                                          GeneratorConfig=O.DBSCAN_GENERATOR_CONFIG))[0]["marker"] == "DBSCAN"
    assert M.compute_outline_box(seq, str(tmp_path), M.MFCF_CONFIG)[0]["marker"] == "MFCF"
    with pytest.raises(NotImplementedError, match="OYSTER"):
        M.compute_outline_box(seq, str(tmp_path), dict(InitLabelGenerator="OYSTER"))
    with pytest.raises(NotImplementedError, match="LabelRefiner"):
        M.compute_outline_box(seq, str(tmp_path), dict(LabelRefiner="OTHER"))
    assert M.compute_outline_box(seq, str(tmp_path), {}) is None
    # outline's own dispatcher keeps its narrower contract
    with pytest.raises(NotImplementedError, match="MFCF"):
        O.compute_outline_box(seq, str(tmp_path), M.MFCF_CONFIG)


def test_dispatcher_runs_the_refiner_after_the_generator(tmp_path, monkeypatch):
    from cpd_amd import cproto_refine
    from cpd_amd import mfcf as M
    calls = []

    class FakeRefiner:
        def __init__(self, seq_name, root_path, cfg):
            calls.append(("init", seq_name))

        def __call__(self):
            calls.append(("call",))
            return "refined"

    monkeypatch.setattr(cproto_refine, "C_PROTO", FakeRefiner)
    seq = "segment-00000004_x"
    os.makedirs(os.path.join(str(tmp_path), seq))
    with open(os.path.join(str(tmp_path), seq, seq + "_outline_MFCF.pkl"), "wb") as f:
        pickle.dump([dict(marker="MFCF")], f)
    cfg = dict(M.MFCF_CONFIG, LabelRefiner="C_PROTO")
    assert M.compute_outline_box(seq, str(tmp_path), cfg) == "refined"
    assert calls == [("init", seq), ("call",)]


def test_generator_config_is_the_yamls():
    from cpd_amd.mfcf import MFCF_GENERATOR_CONFIG as C
    typed = dict(   # GeneratorConfig of waymo_unsupervised_cproto.yaml, typed again by hand
        frame_num=5, frame_interval=1, ppscore_thresh=0.7, sensor_height=0, ground_min_threshold=[0.2, -0.5, -0.5],
        ground_min_distance=[0, 20, 40, 100], ground_max_threshold=1, cluster_dis=0.5, cluster_min_points=5,
        discard_max_height=4, min_box_volume=0.1, min_box_height=0.3, max_box_volume=200, max_box_len=10,
        state_func_covariance=10, measure_func_covariance=0.1, prediction_score_decay=0.025, LiDAR_scanning_frequency=10,
        max_prediction_num=16, max_prediction_num_for_new_object=3, lwh_win_size=0, yaw_win_size=0, smoothing_method='mean',
        cls={'Dis_Small': 0, 'Vehicle': 1, 'Pedestrian': 2, 'Cyclist': 3, 'Dis_Large': 4},
        cls_L={'Dis_Small': [0, 12], 'Vehicle': [0.5, 8], 'Pedestrian': [0.2, 1.], 'Cyclist': [1.3, 2.5], 'Dis_Large': [0, 12]},
        cls_W={'Dis_Small': [0, 12], 'Vehicle': [0.5, 3], 'Pedestrian': [0.2, 1.], 'Cyclist': [0.5, 1.], 'Dis_Large': [0, 12]},
        cls_H={'Dis_Small': [0, 0.8], 'Vehicle': [1., 3], 'Pedestrian': [0.8, 2.3], 'Cyclist': [1.4, 2.], 'Dis_Large': [3, 12]},
        max_top_z=3, max_width=3, max_len=12, input_score=-0.5, init_score=-0.5, update_score=-0.5, post_score=1.4, latency=-1,
        remove_short_track=0)
    assert C == typed
