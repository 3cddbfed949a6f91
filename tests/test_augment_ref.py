"""CPU checks of the training-time augmentor: tests/ref_augment.py's restatement of the two kernels, and cpd_amd.augmentor's
host logic running on it, against the reference's own outputs in tests/golden/augment.npz (make_golden_augment.py)."""
import numpy as np
import pytest

import ref_augment as RA


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


def test_fma32_is_a_fused_multiply_add():
    a = np.float32(1 + 2.0 ** -12)
    # a * a = 1 + 2^-11 + 2^-24 exactly: unfused, the product rounds to 1 + 2^-11 (a tie, to even) and the sum is 0
    assert RA.fma32(a, a, -np.float32(1 + 2.0 ** -11)) == np.float32(2.0 ** -24)
    rng = np.random.default_rng(0)
    x, y, c = (rng.uniform(-80, 80, 100000).astype(np.float32) for _ in range(3))
    ref = (x.astype(np.longdouble) * y.astype(np.longdouble) + c.astype(np.longdouble))
    got = RA.fma32(x, y, c)
    assert (np.abs(got.astype(np.longdouble) - ref) <= np.spacing(np.abs(got)) / 2).all()


def test_forward_restatement_matches_reference(z, drive, database):
    frames, infos = drive
    with RA.host_kernels() as A:
        seen = 0
        for si, d, pasted, _ in RA.replay_scenes(A, z, frames, infos, database, "cpu"):
            RA.check_forward_scene(z, si, d, pasted)
            seen += 1
    assert seen == len(z["scenes"]) == 6
    assert any(bool(z["s%d_flip" % i]) for i in range(6)) and not all(bool(z["s%d_flip" % i]) for i in range(6))


def test_unrotated_restatement_is_the_reference_bit_for_bit(z, drive, database):
    frames, infos = drive
    with RA.host_kernels() as A:
        RA.check_unrotated(z, RA.replay_unrotated(A, z, frames, infos, database, "cpu"))


def test_prepare_train_points_restatement_matches_reference(z, drive, database):
    frames, infos = drive
    with RA.host_kernels() as A:
        for si, d, pasted, perm in RA.replay_scenes(A, z, frames, infos, database, "cpu", prepare=True):
            RA.check_prepared_scene(z, si, d, pasted, perm)


def test_resident_restatement_is_identical(z, drive, database):
    frames, infos = drive
    with RA.host_kernels() as A:
        a = [d for _, d, _, _ in RA.replay_scenes(A, z, frames, infos, database, "cpu", resident=False)]
        b = [d for _, d, _, _ in RA.replay_scenes(A, z, frames, infos, database, "cpu", resident=True)]
    for x, y in zip(a, b):
        assert np.array_equal(x["points"], y["points"]) and np.array_equal(x["gt_boxes"], y["gt_boxes"])


def test_database_restatement_matches_golden(z, drive, tmp_path):
    frames, infos = drive
    with RA.host_kernels() as A:
        db = A.create_track_groundtruth_database(infos, tmp_path, tmp_path, RA.CLASSES, get_lidar=lambda s, i: frames[i].copy(), device="cpu")
    RA.check_database(z, infos, db, tmp_path)


def test_backward_boxes_match_reference(z):
    from cpd_amd import augmentor as A
    for vi, (rot, axis) in enumerate(RA.TEST_VIEWS):
        ta = A.TestAugmentor(RA.test_view_config(rot, axis), RA.CLASSES, num_frames=1)
        got = ta.backward(dict(boxes_lidar=z["view_boxes_in"].copy()))["boxes_lidar"]
        RA.check_boxes(got, z["view%d_back" % vi], "view %d" % vi, rotated=rot != 0)


def test_unsupported_configs_raise(database):
    from cpd_amd import augmentor as A
    for name in ["da_sampling", "random_local_flip", "random_local_noise", "random_local_pyramid_aug", "random_world_trans"]:
        with pytest.raises(NotImplementedError):
            A.DataAugmentor(database, [dict(NAME=name)], RA.CLASSES)
    with pytest.raises(NotImplementedError):
        A.DataAugmentor(database, [], RA.CLASSES, num_frames=2)
    with pytest.raises(NotImplementedError):
        A.TestAugmentor(RA.test_view_config(0, "x"), RA.CLASSES, num_frames=2)
    for key in ["USE_ROAD_PLANE", "USE_VAN", "DATABASE_WITH_FAKELIDAR"]:
        cfg = RA.sampler_config()
        cfg[key] = True
        with pytest.raises(NotImplementedError):
            A.DataBaseSampler(database, cfg, RA.CLASSES, 1, device="cpu")
    with pytest.raises(NotImplementedError):
        A.DataBaseSampler(database, RA.sampler_config(), RA.CLASSES, 2, device="cpu")
    cfg = RA.sampler_config()
    cfg["PREPARE"] = dict(filter_by_min_points=["Vehicle:100000"])
    with pytest.raises(ValueError):
        A.DataBaseSampler(database, cfg, RA.CLASSES, 1, device="cpu")
    with pytest.raises(ValueError):
        A.global_scaling(np.zeros((1, 7), np.float32), None, [1.0, 1.0005])
