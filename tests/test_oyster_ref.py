"""CPU checks of the OYSTER generator (cpd_amd.oyster): the numpy restatement (tests/ref_oyster.py) against the reference's golden
(tests/golden/oyster.npz, made by make_golden_oyster.py) for both runs, the behaviour list one hand-built case each, the host half
of the driver, the dispatcher and the config -- no GPU anywhere."""
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_golden_oyster as MG  # noqa: E402
import ref_oyster as RO  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "oyster.npz")))


@pytest.fixture(scope="module")
def drive(gold):
    infos = MG.box_drive(int(gold["seed"]), int(gold["n_frames_b"]))
    assert MG.drive_digest(infos) == str(gold["digest_b"]), "make_golden_oyster.box_drive no longer gives the golden's input"
    return infos


def _check(got, want, atol=1e-9):
    diff = MG.same_infos(got, want, atol)
    assert diff is None, diff


# ---- the restatement against the reference ---------------------------------------------------------------------------------------

def test_restatement_reproduces_run_a(gold):
    """The point branch: the reference's raw per-frame boxes through cpd_amd.tracker and the restatement."""
    frames, poses = MG.sequence_a(int(gold["seed"]))
    assert MG.digest(frames, poses) == str(gold["digest_a"]), "synthetic.ppscore_sequence no longer gives the golden's input"
    n = int(gold["n_frames_a"])
    stats = {}
    got = RO.generate([MG.frame_boxes(gold, i) for i in range(n)], poses, MG.config_a()["GeneratorConfig"], stats)
    _check(got, MG.unpack_infos(gold, "fina", n))
    counts = dict(zip(gold["counts_keys"].tolist(), gold["counts_vals"].tolist()))
    assert stats["lengths"] == gold["lengths_a"].tolist() and counts["kept_tracks_a"] >= 3
    assert counts["dropped_small_a"] == stats["dropped_small"] >= 1


def test_restatement_reproduces_run_b(gold, drive):
    """The box branch, OYSTER's yaml config unchanged; the golden's counts are what the issue asks of it."""
    from cpd_amd.oyster import OYSTER_GENERATOR_CONFIG
    stats = {}
    got = RO.generate([i['outline_box'] for i in drive], [i['pose'] for i in drive], OYSTER_GENERATOR_CONFIG, stats)
    _check(got, MG.unpack_infos(gold, "finb", len(drive)))
    assert stats["lengths"] == gold["lengths_b"].tolist()
    lengths = gold["lengths_a"].tolist() + gold["lengths_b"].tolist()
    assert 5 in lengths and 6 in lengths and max(lengths) >= 80 and any(60 <= n < 80 for n in lengths)
    assert stats["lone_frames"] >= 1 and stats["empty_frames"] >= 1
    assert stats["dropped_small"] >= 1 and stats["dropped_large"] >= 1 and stats["tied_dis"] == 0
    assert min(stats["corner"]) >= 1


# ---- the behaviour list, one hand-built case each --------------------------------------------------------------------------------

def _box(k, i, l=4.5, w=1.9):
    """Track k in frame i: a box on a circle of its own, moving with i."""
    a = 0.9 * k + 0.01 * i
    return [(12 + 3 * k) * np.cos(a), (12 + 3 * k) * np.sin(a) + 0.1 * i, 0.8, l + 0.01 * i, w + 0.02 * k, 1.6, 0.3 * k]


def _frame(i, ids, cls=None):
    ids = list(ids)
    cls = cls or ['Vehicle'] * len(ids)
    return (np.array([_box(k, i) for k in ids], np.float64).reshape(-1, 7), np.array(ids, np.int64), np.array(cls),
            np.ones(len(ids), np.int64))


class _Tracker:
    """Stands in for TrackSmooth after tracking(): hands out hand-built frames."""

    def __init__(self, frames):
        self.frames = frames

    def get_current_frame_objects_and_cls(self, i):
        return tuple(np.array(v) for v in self.frames[i])


def _driver_host_half(frames):
    """cpd_amd.oyster's collection and regrouping around the restatement's alignment (the kernel's stand-in on the CPU)."""
    from cpd_amd import oyster as O
    tracks = O.collect_tracks(_Tracker(frames), len(frames))
    for t in tracks.values():
        if len(t) >= O.MIN_TRACK_LEN:
            for e, b in zip(t.values(), RO.align_track(np.array([e[0] for e in t.values()]))):
                e[0] = b
    return O.write_frames([dict() for _ in frames], tracks)


def _both(frames):
    got = RO.after_tracker(frames)
    host = _driver_host_half(frames)
    for g, h in zip(got, host):
        for k in ('outline_box', 'outline_ids', 'outline_cls', 'outline_dif'):
            assert g[k].dtype == h[k].dtype and g[k].shape == h[k].shape, k
            np.testing.assert_array_equal(g[k], h[k])
    return got


def test_a_track_of_five_is_dropped_and_one_of_six_is_kept():
    frames = [_frame(i, [0, 1, 2] if i < 5 else [0, 2]) for i in range(6)]        # id 1: five entries; ids 0 and 2: six
    out = _both(frames)
    for i in range(6):
        assert out[i]['outline_ids'].tolist() == [0, 2]
    assert all(1 not in o['outline_ids'] for o in out)


def test_a_frames_only_object_is_lost():
    # frames 0..6 hold ids 0 and 1; frame 3 keeps only id 0 once the Dis_Small box is dropped; frame 7 holds id 0 alone
    frames = [_frame(i, [0, 1]) for i in range(8)]
    frames[3] = _frame(3, [0, 1], ['Vehicle', 'Dis_Small'])
    frames[7] = _frame(7, [0])
    out = _both(frames)
    assert [len(o['outline_ids']) for o in out] == [2, 2, 2, 0, 2, 2, 2, 0]
    # one more lone frame and both tracks fall to five entries: nothing is left
    frames[4] = _frame(4, [0, 1], ['Vehicle', 'Dis_Large'])
    assert [len(o['outline_ids']) for o in _both(frames)] == [0] * 8


def test_rows_follow_the_first_appearance_of_their_track():
    orders = [[5, 2], [2, 5, 9], [9, 2, 5], [2, 9, 5], [5, 9, 2], [9, 5, 2], [2, 5, 9]]
    out = _both([_frame(i, ids) for i, ids in enumerate(orders)])
    assert out[0]['outline_ids'].tolist() == [5, 2]
    for i in range(1, 7):
        assert out[i]['outline_ids'].tolist() == [5, 2, 9]                        # never the detection order
    assert out[2]['outline_box'][0, 5] == 1.6 and out[2]['outline_ids'].dtype == np.int64


def test_empty_frames_have_the_references_shapes_and_dtypes():
    frames = [_frame(i, [0, 1]) for i in range(6)] + [_frame(6, []), _frame(7, [0])]
    out = _both(frames)
    for i in (6, 7):
        assert out[i]['outline_box'].shape == (0, 7) and out[i]['outline_box'].dtype == np.float64
        for k in ('outline_ids', 'outline_cls', 'outline_dif'):
            assert out[i][k].shape == (0,) and out[i][k].dtype == np.float64
    assert out[0]['outline_box'].shape == (2, 7) and out[0]['outline_cls'].dtype.kind == 'U'


@pytest.mark.parametrize("n,top", [(6, 3), (60, 3), (79, 3), (80, 4), (100, 5)])
def test_top_len(n, top):
    from cpd_amd import oyster as O
    assert RO.top_len(n) == O.track_top(n) == top
    assert 1 - 0.95 != 0.05                                                       # Python's factor is 0.050000000000000044
    # the consensus is the mean over exactly that many nearest rows, added in rank order
    rng = np.random.default_rng(n)
    b = np.concatenate([rng.uniform(-30, 30, (n, 2)), rng.uniform(0, 1, (n, 1)), rng.uniform(1, 5, (n, 3)),
                        rng.uniform(-3, 3, (n, 1))], 1)
    near = np.argsort(np.linalg.norm(b[:, 0:3], axis=-1), kind="stable")[:top]
    want = b[near][:, 3:5].mean(axis=0)
    np.testing.assert_array_equal(RO.consensus(b), want)
    if top < n:
        assert RO.consensus(b)[0] != b[np.argsort(np.linalg.norm(b[:, 0:3], axis=-1))[:top + 1]][:, 3].mean()


def _matrix_corner_align(box, l_off, w_off):
    """corner_align as the behaviour list words it: a float32 pose matrix, four homogeneous candidates, the greatest norm."""
    m = np.zeros((4, 4), np.float32)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(box[6]), -np.sin(box[6]), np.sin(box[6]), np.cos(box[6])
    m[0, 3], m[1, 3], m[2, 3], m[2, 2], m[3, 3] = box[0], box[1], box[2], 1, 1
    cand = np.array([[sx * l_off / 2, sy * w_off / 2, 0, 1] for sx, sy in RO.SIGNS])
    moved = cand @ m.T
    k = int(np.argmax(np.linalg.norm(moved, axis=-1)))
    out = np.array(box, np.float64)
    out[3], out[4], out[0:3] = out[3] + l_off, out[4] + w_off, moved[k, 0:3]
    return out, k


def test_corner_align_takes_the_farthest_candidate():
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(200):
        box = np.concatenate([rng.uniform(-40, 40, 2), rng.uniform(0.3, 1.5, 1), rng.uniform(1, 6, 3), rng.uniform(-4, 4, 1)])
        l_off, w_off = rng.uniform(-1, 1, 2)
        got, k = RO.corner_align(box, l_off, w_off, return_choice=True)
        want, kw = _matrix_corner_align(box, l_off, w_off)
        assert k == kw
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        px, py, tz, norm = RO.candidates(box[None], [l_off], [w_off])
        assert norm[k, 0] == norm.max() and norm[k, 0] > norm.min()               # the reference's arg_min is an argmax
        seen.add(k)
    assert seen == {0, 1, 2, 3}


def test_the_first_candidate_wins_ties():
    boxes, off, allowed = RO.tie_tracks()
    for t, (a, b) in enumerate(zip(off[:-1], off[1:])):
        out, choice = RO.align_track(boxes[a:b], return_choice=True)
        mean_l, mean_w = RO.consensus(boxes[a:b])
        if t in (0, 2):
            assert (mean_l - boxes[a:b, 3] == 0).all()
        if t in (1, 2):
            assert (mean_w - boxes[a:b, 4] == 0).all()
        assert set(choice.tolist()) == set(allowed[t]), "track %d" % t             # never the later twin of a tied pair
        for r in range(a, b):
            want, kw = _matrix_corner_align(boxes[r], mean_l - boxes[r, 3], mean_w - boxes[r, 4])
            assert kw == choice[r - a]
            np.testing.assert_allclose(out[r - a], want, rtol=0, atol=1e-12)
    a, b = off[2], off[3]
    out = RO.align_track(boxes[a:b])
    np.testing.assert_array_equal(out[:, [3, 4, 5, 6]], boxes[a:b][:, [3, 4, 5, 6]])
    np.testing.assert_array_equal(out[:, 0:3], boxes[a:b, 0:3].astype(np.float32).astype(np.float64))


def test_z_comes_back_as_float32():
    box = np.array([10.0, -4.0, 0.1, 4.0, 2.0, 1.5, 0.3])
    out = RO.corner_align(box, 0.2, -0.1)
    assert out[2] == np.float64(np.float32(0.1)) != 0.1
    assert out[5] == 1.5 and out[6] == 0.3 and out[3] == 4.0 + 0.2 and out[4] == 2.0 + -0.1
    track = np.array([_box(0, i) for i in range(7)])
    track[:, 2] = 0.1 + 0.01 * np.arange(7)
    np.testing.assert_array_equal(RO.align_track(track)[:, 2], track[:, 2].astype(np.float32).astype(np.float64))


# ---- the driver's host half, the dispatcher, the config --------------------------------------------------------------------------

def test_driver_host_half_on_run_b(gold, drive, tmp_path, monkeypatch):
    """OYSTER() over the hand-built pickle with the launch replaced by the restatement: the file contract, the box branch (no
    frame file exists, none is read), no cache."""
    from cpd_amd import oyster as O
    root = str(tmp_path)
    MG.write_box_drive(root, drive)
    calls = []

    def host_align(boxes, off, device=None):
        calls.append(len(off) - 1)
        assert [O.track_top(int(k)) for k in np.diff(off)] == [RO.top_len(int(k)) for k in np.diff(off)]
        return RO.align_tracks(boxes, off)

    monkeypatch.setattr(O, "align_tracks", host_align)
    monkeypatch.setattr(O.outline.OutlineGPU, "frames_boxes", lambda *a, **k: pytest.fail("no frame needs the per-frame chain"))
    want = MG.unpack_infos(gold, "finb", len(drive))
    infos = O.OYSTER(MG.SEQ_B, root, O.OYSTER_CONFIG)()
    _check(infos, want)
    assert all('pose' in i for i in infos) and calls == [sum(1 for n in gold["lengths_b"] if n >= 6)]
    out_pkl = os.path.join(root, MG.SEQ_B, MG.SEQ_B + "_outline_OYSTER.pkl")
    with open(out_pkl, "rb") as f:
        _check(pickle.load(f), want)
    with open(out_pkl, "wb") as f:                                    # an existing output is not an answer: it is overwritten
        pickle.dump([dict(marker="stale")], f)
    _check(O.create_oyster([MG.SEQ_B], root, O.OYSTER_CONFIG)[0], want)
    with open(out_pkl, "rb") as f:
        _check(pickle.load(f), want)
    assert len(calls) == 2


def test_align_tracks_checks_its_offsets_on_the_host():
    from cpd_amd import _lib
    from cpd_amd import oyster as O
    boxes = np.zeros((8, 7))
    for off in ([0, 5, 3, 8], [1, 8], [0, 7]):
        with pytest.raises(_lib.CpdHipError, match="CPD_ERR_ARG"):
            O.align_tracks(boxes, np.array(off))
    with pytest.raises(ValueError):
        O.align_tracks(boxes, np.array([0.0, 8.0]))
    assert O.align_tracks(np.zeros((0, 7)), np.array([0])).shape == (0, 7)      # T = 0: nothing to launch
    lib = _lib.lib()
    assert lib.cpd_oyster_align_tracks(None, None, None, 0, 0, None, None) == 0
    assert lib.cpd_oyster_align_tracks(None, None, None, 3, 0, None, None) == 0
    assert lib.cpd_oyster_align_tracks(None, None, None, -1, 8, None, None) == -1
    assert lib.cpd_oyster_align_tracks(None, None, None, 1, 8, None, None) == -1
    with pytest.raises(ValueError, match="chunk"):
        O.OYSTER("s", "/nonexistent", O.OYSTER_CONFIG, chunk=0)


def test_dispatcher(tmp_path, monkeypatch):
    from cpd_amd import cproto_refine
    from cpd_amd import mfcf as M
    from cpd_amd import outline
    from cpd_amd import oyster as O
    root = str(tmp_path)
    seqs = dict(DBSCAN="segment-00000011_x", MFCF="segment-00000012_x", OYSTER="segment-00000013_x")
    for name in ("DBSCAN", "MFCF"):                                   # cached generators: the marker file answers
        os.makedirs(os.path.join(root, seqs[name]))
        with open(os.path.join(root, seqs[name], "%s_outline_%s.pkl" % (seqs[name], name)), "wb") as f:
            pickle.dump([dict(marker=name)], f)
    os.makedirs(os.path.join(root, seqs["OYSTER"]))                   # OYSTER has no cache: an input without objects runs through
    with open(os.path.join(root, seqs["OYSTER"], seqs["OYSTER"] + ".pkl"), "wb") as f:
        pickle.dump([dict(pose=np.eye(4), outline_box=np.empty((0, 7)), marker="OYSTER")], f)
    cfgs = dict(DBSCAN=dict(InitLabelGenerator="DBSCAN", GeneratorConfig=outline.DBSCAN_GENERATOR_CONFIG), MFCF=M.MFCF_CONFIG,
                OYSTER=O.OYSTER_CONFIG)
    for name, cfg in cfgs.items():
        got = O.compute_outline_box(seqs[name], root, cfg)
        assert len(got) == 1 and got[0]["marker"] == name
    assert os.path.exists(os.path.join(root, seqs["OYSTER"], seqs["OYSTER"] + "_outline_OYSTER.pkl"))
    assert got[0]['outline_box'].shape == (0, 7) and got[0]['outline_ids'].shape == (0,)
    with pytest.raises(NotImplementedError, match="SOMETHING"):
        O.compute_outline_box(seqs["MFCF"], root, dict(InitLabelGenerator="SOMETHING"))
    with pytest.raises(NotImplementedError, match="LabelRefiner"):
        O.compute_outline_box(seqs["MFCF"], root, dict(LabelRefiner="OTHER"))
    assert O.compute_outline_box(seqs["MFCF"], root, {}) is None
    calls = []

    class FakeRefiner:
        def __init__(self, seq_name, root_path, cfg):
            calls.append(("init", seq_name))

        def __call__(self):
            calls.append(("call",))
            return "refined"

    monkeypatch.setattr(cproto_refine, "C_PROTO", FakeRefiner)
    assert O.compute_outline_box(seqs["OYSTER"], root, dict(O.OYSTER_CONFIG, LabelRefiner="C_PROTO")) == "refined"
    assert O.compute_outline_box(seqs["MFCF"], root, dict(LabelRefiner="C_PROTO")) == "refined"
    assert calls == [("init", seqs["OYSTER"]), ("call",), ("init", seqs["MFCF"]), ("call",)]
    # the older dispatchers keep their narrower contracts
    for mod in (M, outline):
        with pytest.raises(NotImplementedError, match="OYSTER"):
            mod.compute_outline_box(seqs["OYSTER"], root, O.OYSTER_CONFIG)


def test_generator_config_is_the_yamls():
    from cpd_amd.oyster import OYSTER_CONFIG, OYSTER_GENERATOR_CONFIG as C
    typed = dict(   # GeneratorConfig of waymo_unsupervised_oyster.yaml, typed again by hand
        sensor_height=0, ground_min_threshold=[0.2, -0.5, -0.5], ground_min_distance=[0, 20, 40, 100], ground_max_threshold=1,
        cluster_dis=0.5, cluster_min_points=5, discard_max_height=4, min_box_volume=0.1, min_box_height=0.3, max_box_volume=200,
        max_box_len=10, state_func_covariance=10, measure_func_covariance=0.1, prediction_score_decay=0.025,
        LiDAR_scanning_frequency=10, max_prediction_num=16, max_prediction_num_for_new_object=3, lwh_win_size=20, yaw_win_size=10,
        cls={'Dis_Small': 0, 'Vehicle': 1, 'Pedestrian': 2, 'Cyclist': 3, 'Dis_Large': 4},
        cls_L={'Dis_Small': [0, 12], 'Vehicle': [0.5, 8], 'Pedestrian': [0.2, 1.], 'Cyclist': [1.3, 2.5], 'Dis_Large': [0, 12]},
        cls_W={'Dis_Small': [0, 12], 'Vehicle': [0.5, 3], 'Pedestrian': [0.2, 1.], 'Cyclist': [0.5, 1.], 'Dis_Large': [0, 12]},
        cls_H={'Dis_Small': [0, 0.8], 'Vehicle': [1., 3], 'Pedestrian': [0.8, 2.3], 'Cyclist': [1.4, 2.], 'Dis_Large': [3, 12]},
        max_top_z=3, max_width=3, max_len=12, input_score=-0.5, init_score=-0.5, update_score=-0.5, post_score=1.4, latency=-1,
        remove_short_track=10)
    assert C == typed
    assert OYSTER_CONFIG == dict(InitLabelGenerator='OYSTER', GeneratorConfig=typed)
