"""GPU: cpd_amd.outline (csrc/outline.hip) against the reference's recorded pseudo-labels (tests/golden/outline.npz) and the
numpy restatement (tests/ref_outline.py) on hand-built cases."""
import os
import pickle

import numpy as np
import pytest

import ref_outline as R
from test_outline_ref import golden_frames

pytestmark = pytest.mark.gpu
CFG = None


@pytest.fixture(scope="module")
def O(hip):
    global CFG
    from cpd_amd import outline
    CFG = outline.DBSCAN_GENERATOR_CONFIG
    return outline


@pytest.fixture(scope="module")
def oz(golden):
    return golden("outline")


@pytest.fixture(scope="module")
def frames(oz):
    return golden_frames(oz)


@pytest.fixture(scope="module")
def fitter(O):
    return O.OutlineFitter(**{k: CFG[k] for k in ("sensor_height", "ground_min_threshold", "ground_min_distance",
                                                  "cluster_dis", "cluster_min_points", "discard_max_height",
                                                  "min_box_volume", "min_box_height", "max_box_volume", "max_box_len")})


@pytest.mark.parametrize("f", [0, 1, 2])
def test_ground_matches_golden(oz, frames, fitter, f):
    xyz, src = fitter.remove_ground(frames[f], return_index=True)     # [N, 5] rows: the kernel reads with a row stride
    np.testing.assert_array_equal(src, oz["f%d_order" % f])
    np.testing.assert_array_equal(xyz, frames[f][src, :3].astype(np.float64))


@pytest.mark.parametrize("f", [0, 1, 2])
def test_dbscan_matches_golden(oz, frames, fitter, f):
    xyz = frames[f][oz["f%d_order" % f], :3].astype(np.float64)
    labels, ncl = fitter._labels(xyz)
    np.testing.assert_array_equal(labels, oz["f%d_labels" % f])
    assert ncl == oz["f%d_labels" % f].max() + 1


def _grid(n, step, origin=(10.0, 5.0, 0.5)):
    return np.asarray(origin) + step * np.arange(n)[:, None] * np.array([1.0, 0, 0])


BLOB24 = np.array([[0.0625 * i, 0.0625 * j, 0.0625 * k] for i in range(2) for j in range(4) for k in range(3)])   # 2 x 4 x 3


def dbscan_cases():
    rng = np.random.default_rng(5)
    cases = {}
    # a border point next to two clusters: each blob has one core point reaching out to 0.45 of the middle point
    blob = np.array([[0.0, 0.0625 * j, 0.0625 * k] for j in range(4) for k in range(3)])
    A = np.concatenate([blob + [20.0, 3.0, 0.5], [[20.1, 3.0625, 0.5625]]])
    B = np.concatenate([blob + [21.1, 3.0, 0.5], [[21.0, 3.0625, 0.5625]]])
    cases["border_two_clusters"] = np.concatenate([B, [[20.55, 3.0625, 0.5625]], A])
    # exactly 10 neighbours including itself (core) and 9 (not): points on a line 0.0625 apart (float16 grid)
    step = 0.0625
    line10 = [[30.0 + step * k, 7.0, 0.5] for k in range(10)]
    cases["ten_neighbours"] = np.array(line10, np.float64)
    cases["nine_neighbours"] = np.array(line10[:9], np.float64)
    # pairs at exactly d = eps on the float16 grid (0.5 = 8 steps)
    # (columns of 9 points spanning 0.5 in z, 0.5 apart in x: only the exact-eps pairs make 10 neighbours and link columns)
    cases["exact_eps"] = np.array([[40.0 + 0.5 * k, -9.0, 0.25 + 0.0625 * j] for k in range(12) for j in range(9)])
    # duplicate points
    cases["duplicates"] = np.repeat(np.array([[50.0, 1.0, 0.5], [50.3, 1.0, 0.5]]), 6, 0).astype(np.float64)
    cases["all_noise"] = np.float32(rng.uniform(-40, 40, (300, 3)) * [1, 1, 0.01]).astype(np.float64)
    cases["empty"] = np.zeros((0, 3))
    # the shared grid (csrc/hash_grid.h): cells 2 and 2 + 2^18 of side 0.5 share a slot; every candidate is still decided by
    # its distance, so two clumps 2^17 apart are two clusters, and twelve rows in one slot, six in each place, are not core
    blob24 = BLOB24 + [1.0, 1.0, 0.5]
    far = [2.0 ** 17, 0.0, 0.0]
    cases["alias_two_clusters"] = np.concatenate([blob24, blob24 + far])
    cases["alias_not_core"] = np.concatenate([blob24[:6], blob24[:6] + far])
    # cells -1 and 0 on all three axes: floor, not truncation
    cases["negative_cells"] = np.array([[0.0625 * i, 0.0625 * j, 0.0625 * k] for i in range(-2, 2) for j in range(-2, 2)
                                        for k in range(-1, 1)])
    return {k: v.astype(np.float32).astype(np.float64) for k, v in cases.items()}   # float32 values, as remove_ground gives


@pytest.mark.parametrize("name", list(dbscan_cases()))
def test_dbscan_hand_built(fitter, name):
    xyz = dbscan_cases()[name]
    want = R.dbscan_labels(xyz, 0.5)
    got, ncl = fitter._labels(xyz)
    np.testing.assert_array_equal(got, want)
    if name == "border_two_clusters":
        assert want.max() == 1 and want[13] == 0      # the middle point joins the lower-numbered cluster
    if name in ("ten_neighbours", "exact_eps"):
        assert (want >= 0).any()
    if name == "exact_eps":
        assert want.max() == 0 and (want == 0).all()
    if name in ("nine_neighbours", "all_noise", "empty", "alias_not_core"):
        assert (want == -1).all() and ncl == 0
    if name == "alias_two_clusters":
        assert (want[:24] == 0).all() and (want[24:] == 1).all() and ncl == 2
    if name == "negative_cells":
        assert len(want) == 32 and (want == 0).all() and ncl == 1


def test_dbscan_frames_do_not_mix(fitter):
    """Two frames in one launch share the grid and differ only in the tag of their keys: the same cell of two frames must not
    pool its rows."""
    import torch
    g = fitter.gpu
    blob = (BLOB24 + [1.0, 1.0, 0.5]).astype(np.float32)
    for rows, want_label, want_ncl in ((blob, 0, [1, 1]), (blob[:6], -1, [0, 0])):
        n = len(rows)
        xyz = torch.from_numpy(np.concatenate([rows, rows])).to(g.device)
        off = torch.tensor([0, n, 2 * n], dtype=torch.int32, device=g.device)
        cnt = torch.tensor([n, n], dtype=torch.int32, device=g.device)
        labels, ncl = g.dbscan(xyz, off, cnt, 2)
        assert (labels[:2 * n].cpu().numpy() == want_label).all()
        assert ncl.cpu().numpy().tolist() == want_ncl


def test_dbscan_dense_blob(fitter):
    rng = np.random.default_rng(9)
    xyz = np.float32(np.array([15.0, -4.0, 1.0]) + rng.uniform(-0.4, 0.4, (20000, 3))).astype(np.float64)
    labels, ncl = fitter._labels(xyz)
    assert ncl == 1 and (labels == 0).all()


@pytest.mark.parametrize("f", [0, 1, 2])
def test_boxes_match_golden(oz, frames, fitter, f):
    p = "f%d_" % f
    xyz = frames[f][oz[p + "order"], :3].astype(np.float64)
    clusters, _ = fitter.clustering(xyz)
    cbox, cflag = oz[p + "cbox"], oz[p + "cflag"]
    assert len(clusters) == len(cbox)
    n_fit = 0
    for i, c in enumerate(clusters):
        b = fitter.box_fit([c])
        n_fit += len(b) > 0
        if cflag[i]:
            continue
        if len(b) == 0:
            assert np.isnan(cbox[i]).all(), i
        else:
            assert np.abs(b[0] - cbox[i]).max() <= 1e-9, (i, b[0], cbox[i])
    assert n_fit == int(np.isfinite(cbox[:, 0]).sum())
    print("frame %d: %d of %d kept clusters flagged (%.0f %%)" % (f, int((cflag != 0).sum()), len(cflag),
                                                                  100.0 * (cflag != 0).mean()))


def test_degenerate_and_large_clusters(fitter):
    rng = np.random.default_rng(3)
    collinear = np.array([[10.0 + 0.25 * k, 2.0 + 0.125 * k, 0.5 + 0.5 * (k % 3)] for k in range(30)], np.float64)
    two = np.array([[5.0, 5.0, 0.0]] * 10 + [[5.0, 5.25, 1.0], [5.5, 5.0, 1.0]], np.float64)
    big = np.float32(np.c_[rng.uniform(20, 24, 24000), rng.uniform(-3, -1, 24000), rng.uniform(0, 1.8, 24000)])
    big = big.astype(np.float64)
    assert len(fitter.box_fit([collinear])) == 0
    assert len(fitter.box_fit([two])) == 0
    got = fitter.box_fit([big])
    want = R.box_fit([big], CFG)
    assert len(got) == 1 and np.abs(got[0] - want[0]).max() <= 1e-9


def test_final_arrays_match_golden(O, oz, frames):
    res = O.outline_frames(frames, CFG)
    for f, (b, cls, dif) in enumerate(res):
        p = "f%d_" % f
        np.testing.assert_array_equal(cls, oz[p + "cls"])
        np.testing.assert_array_equal(dif, oz[p + "dif"])
        assert b.shape == oz[p + "box"].shape
        if not oz[p + "cflag"].any():
            assert np.abs(b - oz[p + "box"]).max() <= 1e-9


def test_batching_and_repeatability(O):
    from cpd_amd.synthetic import outline_scene
    fr = [outline_scene(100 + k, np.float16 if k % 2 else np.float32, n_az=600) for k in range(8)]
    fr = [f.astype(np.float16) for f in fr]
    g = O.OutlineGPU(O._params(CFG))
    batch = g.frames_boxes(fr)
    again = g.frames_boxes(fr)
    single = [g.frames_boxes([f])[0] for f in fr]
    assert sum(len(b) for b in batch) > 0
    for x, y, z in zip(batch, again, single):
        assert np.array_equal(np.asarray(x), np.asarray(y)) and np.array_equal(np.asarray(x), np.asarray(z))


def test_sequence_driver_and_cache(O, oz, frames, tmp_path):
    seq = "segment-test"
    d = tmp_path / seq
    d.mkdir()
    idx = [0, 2]                                    # the float16 golden frames, saved as Waymo frames are
    for i, f in enumerate(idx):
        np.save(d / ("%04d.npy" % i), frames[f])
    with open(d / (seq + ".pkl"), "wb") as fh:
        pickle.dump([{"frame_id": i} for i in range(len(idx))], fh)
    cfg = dict(InitLabelGenerator="DBSCAN", GeneratorConfig=CFG)
    infos = O.create_outline_boxes([seq], str(tmp_path), cfg)[0]
    out = d / (seq + "_outline_DBSCAN.pkl")
    assert out.exists()
    for i, f in enumerate(idx):
        p = "f%d_" % f
        np.testing.assert_array_equal(infos[i]["outline_cls"], oz[p + "cls"])
        np.testing.assert_array_equal(infos[i]["outline_dif"], oz[p + "dif"])
        assert infos[i]["outline_box"].shape == oz[p + "box"].shape
        if not oz[p + "cflag"].any():
            assert np.abs(infos[i]["outline_box"] - oz[p + "box"]).max() <= 1e-9
    mtime = os.path.getmtime(out)
    again = O.DBSCAN(seq, str(tmp_path), cfg)()
    assert os.path.getmtime(out) == mtime
    assert len(again) == len(idx) and np.array_equal(again[0]["outline_cls"], infos[0]["outline_cls"])
