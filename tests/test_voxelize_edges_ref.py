"""CPU checks of tests/ref_voxelize_edges.py: every scene of the voxelizer edge tests really contains the edge it is named for,
counted with the C oracle's serial voxelizer and with the scenes module's own cell keys. A GPU test of
tests/test_gpu_voxelize_edges.py therefore cannot pass by missing its edge."""
import numpy as np
import pytest

import ref_voxelize_edges as R


def _oracle(oracle, sc):
    return oracle.voxelize(sc["points"], sc["voxel_size"], sc["point_cloud_range"], sc["P"], sc["max_voxels"])


def _geo(sc):
    return dict(voxel_size=sc["voxel_size"], point_cloud_range=sc["point_cloud_range"])


def _cell_counts(sc):
    keys = R.cell_keys(sc["points"], _geo(sc))
    return keys, np.unique(keys[keys >= 0], return_counts=True)


def test_scenes_are_small_and_the_keys_are_the_oracles(oracle):
    assert R.grid_zyx(R.GRID).tolist() == oracle.grid_size(R.GRID["voxel_size"], R.GRID["point_cloud_range"]) == [4, 8, 8]
    assert R.grid_zyx(R.WAYMO).tolist() == oracle.grid_size(R.WAYMO["voxel_size"], R.WAYMO["point_cloud_range"]) == [40, 1504, 1504]
    for name, make in R.SCENES.items():
        sc = make()
        assert len(sc["points"]) <= 2000 and sc["points"].dtype == np.float32, name
        keys, (cells, cnt) = _cell_counts(sc)
        big = dict(sc, P=4096, max_voxels=4096)                  # no cap binds: the oracle's rows are the occupied cells
        _, c0, n0 = _oracle(oracle, big)
        g = R.grid_zyx(_geo(sc))
        k0 = (c0[:, 0].astype(np.int64) * g[1] + c0[:, 1]) * g[2] + c0[:, 2]
        order = np.argsort(k0)
        np.testing.assert_array_equal(k0[order], cells, err_msg=name)
        np.testing.assert_array_equal(n0[order], cnt, err_msg=name)


@pytest.mark.parametrize("n", R.SIZES)
def test_size_scenes_have_invalid_points_and_runs_over_the_wave_and_block_edges(n):
    sc = R.size_scene(n)
    pts = sc["points"]
    assert pts.shape == (n, 4)
    keys = R.cell_keys(pts, R.GRID)
    if n >= 63:
        bad = keys < 0
        assert 0.04 * n <= bad.sum() <= 0.16 * n
        xyz = pts[bad, :3]
        assert np.isnan(xyz).any() and np.isposinf(xyz).any() and (np.isneginf(xyz).any() or n < 255)
        assert (np.isfinite(xyz).all(1)).any()                   # ... and finite points outside the range
        assert keys[0] >= 0 and keys[1] == keys[0]               # lane 0 starts a run
        runs = (keys[1:] == keys[:-1]) & (keys[1:] >= 0)
        assert runs.sum() > n // 4
    for edge in (R.WAVE, R.BLOCK, 4 * R.BLOCK):
        if edge < n:                                             # the run crosses into the next wave / block
            assert keys[edge - 1] >= 0 and keys[edge - 2] == keys[edge - 1] == keys[edge]
    # the sizes sit on both sides of a wave and of a block, and one of them ends a point past the fourth block
    assert {n - R.WAVE for n in R.SIZES} >= {-1, 0, 1} and {n - R.BLOCK for n in R.SIZES} >= {-1, 0, 1} and 4 * R.BLOCK + 1 in R.SIZES


def test_one_voxel_scenes_exceed_max_points(oracle):
    sc = R.one_voxel()
    keys, (cells, cnt) = _cell_counts(sc)
    assert len(cells) == 1 and cnt[0] == 200 > sc["P"] == 5
    v, c, n = _oracle(oracle, sc)
    assert len(c) == 1 and n[0] == 5
    np.testing.assert_array_equal(v[0], sc["points"][:5])       # the first P points in point order
    sc = R.one_voxel_run()
    keys, (cells, cnt) = _cell_counts(sc)
    run = np.flatnonzero(keys == 91)
    assert run[0] == 50 and (keys[50:150] == 91).all() and len(run) == 103        # lanes 50 .. 63, a whole wave, lanes 0 .. 21; stragglers
    assert run[0] % R.WAVE + sc["P"] < R.WAVE                    # the kept points all sit in the first wave; later waves only count
    v, c, n = _oracle(oracle, sc)
    row = int(np.flatnonzero((c == [1, 3, 3]).all(1))[0])        # cell 91 = (z 1, y 3, x 3)
    assert n[row] == 5 and 1 < len(c) < 100
    np.testing.assert_array_equal(v[row], sc["points"][50:55])


def test_per_voxel_cap_scenes_sit_below_and_above_every_count(oracle):
    keys, (cells, cnt) = _cell_counts(R.per_voxel_cap(1))
    assert cnt.max() < 35 and (cnt > 1).mean() > 0.8 and cnt.max() > 5
    _, _, n1 = _oracle(oracle, R.per_voxel_cap(1))
    _, _, n35 = _oracle(oracle, R.per_voxel_cap(35))
    assert (n1 == 1).all() and len(n1) == len(n35) == len(cells) and n35.max() == cnt.max() and sorted(n35) == sorted(cnt)


def test_voxel_cap_scenes_exceed_max_voxels(oracle):
    sc = R.every_cell_cap()
    keys, (cells, cnt) = _cell_counts(sc)
    assert len(cells) == 256 and sc["max_voxels"] == 100 and (keys >= 0).all()
    assert len(_oracle(oracle, sc)[1]) == 100
    sc = R.late_voxels_cap()
    keys, (cells, cnt) = _cell_counts(sc)
    assert len(cells) > 150 and (keys < 0).sum() > 50             # half as many voxels again as the cap admits, at least
    v, c, n = _oracle(oracle, sc)
    assert len(c) == 100
    g = R.grid_zyx(R.GRID)
    kept = (c[:, 0].astype(np.int64) * g[1] + c[:, 1]) * g[2] + c[:, 2]
    first = {int(k): int(np.flatnonzero(keys == k)[0]) for k in cells}
    last_kept_start = max(first[int(k)] for k in kept)
    dropped = [k for k in cells if k not in set(kept.tolist())]
    assert all(first[int(k)] > last_kept_start for k in dropped)                  # the dropped voxels are the ones that appear late
    late = np.arange(len(keys)) > last_kept_start
    assert np.isin(keys[late], kept).sum() > 100 and np.isin(keys[late], dropped).sum() > 100
    # ... and a kept voxel still takes points that arrive after the cap was reached (its count is not frozen at that moment)
    early_cnt = np.array([(keys[:last_kept_start + 1] == k).sum() for k in kept])
    assert (n > np.minimum(early_cnt, sc["P"])).any()


def test_empty_scenes_give_no_rows(oracle):
    for sc in (R.no_points(), R.all_outside()):
        v, c, n = _oracle(oracle, sc)
        assert v.shape == (0, 5, 4) and c.shape == (0, 3) and n.shape == (0,)
    sc = R.all_outside()
    assert len(sc["points"]) == 300 and (R.cell_keys(sc["points"], R.GRID) < 0).all()
    xyz = sc["points"][:, :3]
    assert np.isnan(xyz).any() and np.isinf(xyz).any() and np.isfinite(xyz).all(1).any()


def test_waymo_scene_is_a_sparse_bitmap(oracle):
    sc = R.waymo_sparse()
    keys, (cells, cnt) = _cell_counts(sc)
    total = int(np.prod(R.grid_zyx(R.WAYMO)))
    assert total > 9 * 10 ** 7 and len(sc["points"]) == 2000 and 500 < len(cells) < 2000
    assert len(np.unique(cells // (64 * 4096))) > 200            # bits in hundreds of the bitmap scan's 4096-word blocks, most blocks empty
    assert len(_oracle(oracle, sc)[1]) == len(cells)


def test_parameter_scenes():
    assert [R.channels(c)["points"].shape for c in (3, 4, 5)] == [(257, 3), (257, 4), (257, 5)]
    assert sorted(R.COORD_PARAMS) == [(3, 0), (3, 3), (4, 0), (4, 3)]
    assert set(R.RAW_SCENES) <= set(R.SCENES) and len(R.SCENES[R.RAW_SCENES[0]]()["points"]) == 0
