"""GPU checks of the training-time augmentor (csrc/augment.hip, cpd_amd/augmentor.py): the golden scenes of the reference
(tests/golden/augment.npz) and the two kernels at their edges against the numpy restatement (tests/ref_augment.py)."""
import numpy as np
import pytest
import torch

import ref_augment as RA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def A(hip):
    from cpd_amd import augmentor
    return augmentor


@pytest.fixture(scope="module")
def z(golden):
    return golden("augment")


@pytest.fixture(scope="module")
def drive(z):
    return RA.rebuild(z)


@pytest.fixture(scope="module")
def database(z, drive, tmp_path_factory):
    root = tmp_path_factory.mktemp("augment_db")
    RA.write_golden_database(z, drive[1], root)
    return root


@pytest.fixture(scope="module")
def forward_runs(A, z, drive, database):
    """DataAugmentor.forward over the golden scenes, not resident and resident: computed once, shared."""
    frames, infos = drive
    return {res: list(RA.replay_scenes(A, z, frames, infos, database, DEV, resident=res)) for res in (False, True)}


# 1. the golden scenes
def test_forward_matches_reference(z, forward_runs):
    assert len(forward_runs[False]) == 6
    for si, d, pasted, _ in forward_runs[False]:
        RA.check_forward_scene(z, si, d, pasted)


def test_unrotated_scenes_are_the_reference_bit_for_bit(A, z, drive, database):
    frames, infos = drive
    RA.check_unrotated(z, RA.replay_unrotated(A, z, frames, infos, database, DEV))


def test_prepare_train_points_matches_reference(A, z, drive, database):
    frames, infos = drive
    for si, d, pasted, perm in RA.replay_scenes(A, z, frames, infos, database, DEV, prepare=True):
        RA.check_prepared_scene(z, si, d, pasted, perm)


def test_points1_is_masked_and_shuffled_but_not_augmented(A, z, drive):
    frames, infos = drive
    aug = A.DataAugmentor(None, RA.augmentor_config(with_sampling=False), RA.CLASSES)
    gt_boxes, gt_names = RA.frame_labels(infos, 1)
    np.random.seed(5)
    d = A.prepare_train_points(dict(points=torch.from_numpy(frames[1]).to(DEV), points1=torch.from_numpy(frames[2]).to(DEV),
                                    gt_boxes=gt_boxes, gt_names=gt_names), z["pcr"], True, augmentor=aug)
    want = RA.augment_scene(frames[2], limit_range=z["pcr"])
    got = d["points1"].cpu().numpy()
    assert got.shape == want.shape and not np.array_equal(got, want)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    assert np.array_equal(order(got), order(want))


# 2. resident against not resident
def test_resident_is_bit_identical(forward_runs):
    for (_, a, _, _), (_, b, _, _) in zip(forward_runs[False], forward_runs[True]):
        assert a["points"].tobytes() == b["points"].tobytes()
        assert a["gt_boxes"].tobytes() == b["gt_boxes"].tobytes()
        assert np.array_equal(a["gt_names"], b["gt_names"]) and np.array_equal(a["aug_param"], b["aug_param"])


# 3. cpd_augment_scene at its edges
OPS8 = [(RA.FLIP_X, 0, 0), (RA.ROT, np.float32(np.cos(0.7)), np.float32(np.sin(0.7))), (RA.SCALE, 1.0371, 0), (RA.FLIP_Y, 0, 0),
        (RA.ROT, np.float32(np.cos(-2.1)), np.float32(np.sin(-2.1))), (RA.SCALE, 0.9513, 0), (RA.FLIP_X, 0, 0),
        (RA.ROT, np.float32(np.cos(0.05)), np.float32(np.sin(0.05)))]
RANGE = [-15.0, -14.0, -2.0, 16.0, 15.0, 4.0]


def scene_case(rng, n, m, k, c, c_obj):
    scene = rng.uniform(-20, 20, (n, c)).astype(np.float32)
    scene[:, 2] = rng.uniform(-1, 3, n)
    boxes = np.zeros((k, 7), np.float32)
    boxes[:, :2] = rng.uniform(-20, 20, (k, 2))
    boxes[:, 2] = rng.uniform(0, 2, k)
    boxes[:, 3:6] = rng.uniform(0.5, 4, (k, 3)) * (1.0 if k <= 65 else 0.4)
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, k)
    base = rng.uniform(-3, 3, (m + 37, c_obj)).astype(np.float32)
    # segments out of order and overlapping in obj_base; some empty
    start, count, left = [], [], m
    while left > 0:
        cnt = int(min(left, rng.integers(0, 70)))
        st = int(rng.integers(0, base.shape[0] - cnt + 1))
        start.append(st); count.append(cnt)
        left -= cnt
    centre = rng.uniform(-18, 18, (len(start), 3))
    return scene, boxes, base, start, count, centre


def run_both(A, scene, ops, limit_range, base, start, count, centre, boxes):
    got = A.augment_scene(torch.from_numpy(scene).to(DEV), ops, limit_range, torch.from_numpy(base).to(DEV) if base is not None else None,
                          start, count, centre, boxes if boxes is None else torch.from_numpy(boxes)).cpu().numpy()
    want = RA.augment_scene(scene, ops, limit_range, base, start, count, centre, boxes)
    assert got.shape == want.shape, "%s rows, the restatement has %s" % (got.shape, want.shape)
    assert got.tobytes() == want.tobytes()
    return got


@pytest.mark.parametrize("k", [0, 1, 65, 512])
def test_augment_scene_edges(A, k):
    rng = np.random.default_rng(100 + k)
    case = 0
    for n in [0, 1, 63, 64, 65, 255, 256, 257, 1025]:
        for m in [0, 1, 64, 300]:
            c = 4 + case % 3
            c_obj = c + (case // 3) % 2
            scene, boxes, base, start, count, centre = scene_case(rng, n, m, k, c, c_obj)
            ops = OPS8 if case % 2 else []
            rng_ = RANGE if case % 4 < 3 else None
            got = run_both(A, scene, ops, rng_, base, start, count, centre, boxes)
            if n == 1025 and m == 300 and k in (65, 512):
                assert 0 < got.shape[0] < n + m                       # rows are removed and rows are kept
            case += 1


def test_augment_scene_special_rows(A):
    rng = np.random.default_rng(7)
    scene, boxes, base, start, count, centre = scene_case(rng, 700, 130, 3, 5, 6)
    # every scene point inside a box
    big = np.array([[0, 0, 1, 100, 100, 20, 0.3]], np.float32)
    got = run_both(A, scene, OPS8, None, base, start, count, centre, big)
    assert got.shape[0] == 130
    # every row outside the range
    got = run_both(A, scene, [], [50.0, 50.0, 0, 60.0, 60.0, 1], base, start, count, centre, boxes)
    assert got.shape[0] == 0
    # a NaN row: kept without a range (no box contains it), dropped with one
    scene[5, 0] = np.nan
    scene[9, 1] = np.nan
    a = run_both(A, scene, [], None, None, None, None, None, None)
    b = run_both(A, scene, [], [-100.0, -100.0, 0, 100.0, 100.0, 1], None, None, None, None, None)
    assert a.shape[0] == 700 and b.shape[0] == 698
    # nothing at all
    got = run_both(A, scene[:0], [], RANGE, None, None, None, None, None)
    assert got.shape == (0, 5)
    # ROT alone is the fused chain
    got = run_both(A, scene[20:], OPS8[1:2], None, None, None, None, None, None)
    x, y = scene[20:, 0], scene[20:, 1]
    cs, sn = np.float32(OPS8[1][1]), np.float32(OPS8[1][2])
    assert np.array_equal(got[:, 0], RA.fma32(y, -sn, x * cs)) and np.array_equal(got[:, 1], RA.fma32(y, cs, x * sn))


def test_augment_scene_limits(A):
    from cpd_amd._lib import CpdHipError
    scene = torch.zeros((4, 5), device=DEV)
    base = torch.zeros((4, 5), device=DEV)
    with pytest.raises(CpdHipError, match="CPD_ERR_UNSUPPORTED"):
        A.augment_scene(scene, boxes=torch.zeros((513, 7)))
    with pytest.raises(CpdHipError, match="CPD_ERR_UNSUPPORTED"):
        A.augment_scene(scene, obj_base=base, obj_start=[0] * 513, obj_count=[0] * 513, obj_centre=np.zeros((513, 3)))
    with pytest.raises(CpdHipError, match="CPD_ERR_UNSUPPORTED"):
        A.augment_scene(scene, ops=[(RA.FLIP_X, 0, 0)] * 9)
    with pytest.raises(CpdHipError, match="CPD_ERR_UNSUPPORTED"):
        A.augment_scene(scene, obj_base=base, obj_start=[0, 0], obj_count=[2 ** 30, 2 ** 30], obj_centre=np.zeros((2, 3)))
    with pytest.raises(CpdHipError, match="CPD_ERR_ARG"):                 # a segment past the end of obj_base
        A.augment_scene(scene, obj_base=base, obj_start=[2], obj_count=[3], obj_centre=np.zeros((1, 3)))


# 4. cpd_group_points_by_box at its edges
def group_both(A, pts, idx, centres):
    rows, off = A.group_points_by_box(torch.from_numpy(pts).to(DEV), torch.from_numpy(idx).to(DEV), centres)
    off = off.cpu().numpy()
    want_rows, want_off = RA.group_points_by_box(pts, idx, centres)
    assert np.array_equal(off, want_off)
    assert rows[:off[-1]].cpu().numpy().tobytes() == want_rows.tobytes()


@pytest.mark.parametrize("k", [1, 2, 33, 128, 1024])
def test_group_points_by_box_edges(A, k):
    rng = np.random.default_rng(200 + k)
    for case, n in enumerate([1, 64, 65, 256, 257, 4097, 70000]):
        c = 5 + case % 2
        pts = rng.uniform(-60, 60, (n, c)).astype(np.float32)
        centres = rng.uniform(-60, 60, (k, 3))
        patterns = [rng.integers(-1, k, n),                               # random, with background
                    np.arange(n) % k,                                     # round robin: stability across waves and blocks
                    np.full(n, k - 1),                                    # all points in one box
                    np.full(n, -1)]                                       # none in any box
        if k > 2:
            patterns.append(rng.integers(1, k - 1, n))                    # empty first and last boxes
        for idx in patterns if n < 70000 else patterns[:2]:
            group_both(A, pts, idx.astype(np.int32), centres)


def test_group_points_by_box_limit(A):
    from cpd_amd._lib import CpdHipError
    with pytest.raises(CpdHipError, match="CPD_ERR_UNSUPPORTED"):
        A.group_points_by_box(torch.zeros((8, 5), device=DEV), torch.zeros((8,), dtype=torch.int32, device=DEV), np.zeros((1025, 3)))


# 5. the database writer
def test_create_database_matches_golden(A, z, drive, tmp_path):
    frames, infos = drive
    db = A.create_track_groundtruth_database(infos, tmp_path, tmp_path, RA.CLASSES, get_lidar=lambda s, i: frames[i].copy(), device=DEV)
    RA.check_database(z, infos, db, tmp_path)


# 6. the test-time views
def test_test_augmentor_views(A, z, drive):
    frames, _ = drive
    boxes = z["view_boxes_in"]
    for rot, axis in RA.TEST_VIEWS:
        ta = A.TestAugmentor(RA.test_view_config(rot, axis), RA.CLASSES, num_frames=1)
        got = ta.forward(dict(points=torch.from_numpy(frames[0]).to(DEV)))["points"].cpu().numpy()
        cs, sn = A.rotation_cos_sin(rot)
        ops = [(RA.ROT, cs, sn)] + ([(RA.FLIP_X, 0, 0)] if axis == "x" else []) + [(RA.SCALE, 1, 0)]
        want = frames[0].copy()
        want[:, :3] = RA.apply_ops(want[:, :3], ops)
        assert got.tobytes() == want.tobytes()
        # a box table seen through the view -- centres as points are, heading and sign as the view moves them -- comes back
        fwd = boxes.copy()
        ctr = ta.forward(dict(points=torch.from_numpy(np.ascontiguousarray(boxes[:, :5])).to(DEV)))["points"].cpu().numpy()
        fwd[:, :3] = ctr[:, :3]
        fwd[:, 6] = (boxes[:, 6] + np.float32(rot)) * (-1 if axis == "x" else 1)
        back = ta.backward(dict(boxes_lidar=fwd.copy()))["boxes_lidar"]
        RA.assert_xyz_close(back[:, :2], boxes[:, :2], "view (%s, %s) centres" % (rot, axis))
        assert np.array_equal(back[:, 2:6], boxes[:, 2:6])
        assert np.abs(back[:, 6] - boxes[:, 6]).max() <= 2 * np.spacing(np.float32(4.0))
