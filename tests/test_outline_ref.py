"""CPU: the numpy restatement of the DBSCAN pseudo-label generator (tests/ref_outline.py) and cpd_amd.outline's host-side
class chain against the reference's recorded output (tests/golden/outline.npz, written by make_golden_outline.py)."""
import hashlib

import numpy as np
import pytest

import ref_outline as R
from cpd_amd import outline as O
from cpd_amd.synthetic import outline_scene

CFG = O.DBSCAN_GENERATOR_CONFIG


@pytest.fixture(scope="module")
def oz(golden):
    return golden("outline")


def golden_frames(oz):
    """The golden's input frames, regenerated from their seeds and checked against the stored digests."""
    out = []
    for f, (seed, dt) in enumerate(zip(oz["frames_seed"], oz["frames_dtype"])):
        pts = outline_scene(int(seed), np.dtype(str(dt)), n_az=int(oz["n_az"]))
        d = hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest()
        assert d == str(oz["f%d_digest" % f]), ("outline_scene(%d, %s) no longer reproduces the golden's input (numpy RNG "
                                                "or synthetic.py changed): regenerate tests/golden/outline.npz" % (seed, dt))
        out.append(pts)
    return out


@pytest.fixture(scope="module")
def frames(oz):
    return golden_frames(oz)


def test_golden_covers_both_dtypes(oz):
    assert {"float16", "float32"} <= set(map(str, oz["frames_dtype"]))


@pytest.mark.parametrize("f", [0, 1, 2])
def test_restatement_matches_reference(oz, frames, f):
    p = "f%d_" % f
    xyz, src = R.remove_ground(frames[f], CFG, return_index=True)
    np.testing.assert_array_equal(src, oz[p + "order"])
    np.testing.assert_array_equal(xyz, frames[f][src, :3].astype(np.float64))
    labels = R.dbscan_labels(xyz, CFG["cluster_dis"])
    np.testing.assert_array_equal(labels, oz[p + "labels"])
    clusters, _ = R.clustering(xyz, CFG)
    cbox, cflag = oz[p + "cbox"], oz[p + "cflag"]
    assert len(clusters) == len(cbox)
    for i, c in enumerate(clusters):
        b = R.box_fit([c], CFG)
        if cflag[i]:
            continue
        if len(b) == 0:
            assert np.isnan(cbox[i]).all(), i
        else:
            assert np.abs(b[0] - cbox[i]).max() <= 1e-9, i
    print("frame %d: %d of %d kept clusters flagged" % (f, int((cflag != 0).sum()), len(cflag)))


@pytest.mark.parametrize("f", [0, 1, 2])
def test_host_box_cls_and_drop_match_reference(oz, f):
    p = "f%d_" % f
    cbox = oz[p + "cbox"]
    boxes = cbox[np.isfinite(cbox[:, 0])]
    b, cls, dif = O.get_box_cls(boxes, CFG)
    b, cls, _, dif, _, _ = O.drop_cls(b, cls, dif=dif)
    np.testing.assert_array_equal(b, oz[p + "box"])
    np.testing.assert_array_equal(cls, oz[p + "cls"])
    assert cls.dtype == oz[p + "cls"].dtype
    np.testing.assert_array_equal(dif, oz[p + "dif"])
    assert dif.dtype == oz[p + "dif"].dtype


def test_empty_frame_shapes():
    b, cls, dif = O.get_box_cls([], CFG)
    b, cls, _, dif, _, _ = O.drop_cls(b, cls, dif=dif)
    for a in (b, cls, dif):
        assert a.shape == (0,) and a.dtype == np.float64
    assert R.remove_ground(np.zeros((0, 3), np.float16), CFG).shape == (0, 3)
    assert len(R.dbscan_labels(np.zeros((0, 3)), 0.5)) == 0


def test_class_chain_order():
    boxes = np.array([[0, 0, 0, 4.0, 2.0, 1.6, 0],      # Vehicle
                      [0, 0, 0, 0.6, 0.5, 1.7, 0],      # Pedestrian
                      [0, 0, 0, 1.8, 0.7, 1.6, 0],      # Cyclist (Pedestrian's l range fails)
                      [0, 0, 0, 1.0, 1.0, 0.5, 0],      # Dis_Small range first
                      [0, 0, 2.5, 2.0, 2.0, 1.5, 0],    # top_z > max_top_z -> Dis_Large
                      [0, 0, 0, 13.0, 2.0, 1.5, 0],     # l > max_len
                      [0, 0, 0, 9.0, 2.0, 1.5, 0]])     # no range -> Dis_Small
    _, cls, dif = O.get_box_cls(boxes, CFG)
    assert cls.tolist() == ["Vehicle", "Pedestrian", "Cyclist", "Dis_Small", "Dis_Large", "Dis_Large", "Dis_Small"]
    assert dif.tolist() == [1] * 7


def test_other_dtypes_raise():
    with pytest.raises(TypeError):
        O._check_points(np.zeros((4, 3), np.float64))
    with pytest.raises(TypeError):
        R.remove_ground(np.zeros((4, 3), np.float64), CFG)


def test_other_generators_raise():
    with pytest.raises(NotImplementedError, match="OYSTER"):
        O.compute_outline_box("seq", "/nonexistent", dict(InitLabelGenerator="OYSTER"))
    with pytest.raises(NotImplementedError, match="C_PROTO"):
        O.compute_outline_box("seq", "/nonexistent", dict(LabelRefiner="C_PROTO"))
