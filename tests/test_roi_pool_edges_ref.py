"""CPU checks of tests/ref_roi_pool_edges.py: every scene of the RoI-pooling edge tests really contains the edge it is named for
(counted with the C oracle's voxel query), and the float64 pooling / grouping references are the module's definition (against
oracle.group_points and a direct loop). A GPU test of tests/test_gpu_roi_pool_edges.py therefore cannot pass by missing its edge."""
import numpy as np
import pytest

import ref_roi_pool_edges as R

BIG = 512                            # more slots than the largest window has cells (3 * 5 * 31 = 465)


def _counts(oracle, sc, ranges, radius, q, qxyz=None):
    xyz = R.centres(sc, sc["cells"][:, 1:4])
    v2p = oracle.voxel2pinds(sc["cells"], sc["batch"], sc["shape"])
    qxyz = R.centres(sc, q[:, 1:4]) if qxyz is None else qxyz
    return R.hit_counts(oracle.voxel_query(ranges, radius, BIG, xyz, qxyz, q, v2p))


def test_scene_sizes():
    for name, make in R.SCENES.items():
        sc = make()
        cells = sc["batch"] * int(np.prod(sc["shape"]))
        assert cells <= 22560, name
        occ = len(sc["cells"]) / cells
        assert {"dense": occ == 1.0, "sparse": 0.07 < occ < 0.13, "checker": occ == 0.5, "half": occ == 0.5, "far": 0.45 < occ < 0.55}[name]
    # the bitmap's cell count is a multiple of 64 for some word scenes and not for others
    assert {(2 * 2 * 3 * r3) % 64 == 0 for r3 in R.WORDS_R3} == {True, False}


def test_case1_every_nsample_meets_more_equal_fewer_and_no_hits(oracle):
    counts = []
    for name, radius in R.CASE1:
        sc = R.SCENES[name]()
        for ranges in R.RANGES:
            counts.append(_counts(oracle, sc, ranges, radius, R.queries_around(sc, ranges)))
        if name == "dense":                                      # the radius covers the window: a count is the window's in-grid volume
            q = R.queries_around(sc, R.RANGES[2])
            vol = np.prod([np.clip(np.minimum(q[:, 1 + a] + r, s - 1) - np.maximum(q[:, 1 + a] - r, 0) + 1, 0, None)
                           for a, (r, s) in enumerate(zip(R.RANGES[2], sc["shape"]))], axis=0)
            np.testing.assert_array_equal(counts[2], vol)
    counts = np.concatenate(counts)
    for ns in R.NSAMPLES:
        assert (counts > ns).any() and (counts == ns).any() and (counts == 0).any(), ns
        if ns > 1:                                               # (no count lies between 1 and 0)
            assert ((counts >= 1) & (counts < ns)).any(), ns


def test_case2_ragged_waves_mix_full_cut_and_empty_windows(oracle):
    sc = R.half()
    q = R.queries_ragged(sc, 65)
    for ranges in ([1, 2, 15], [1, 1, 16]):
        c = _counts(oracle, sc, ranges, R.RADIUS_ALL, q)
        rows = 3 * (2 * ranges[1] + 1)
        for w in range(0, 64, 4):                                # every wave (4 consecutive queries): an empty window beside one with
            assert (c[w:w + 4] == 0).any() and (c[w:w + 4] > max(R.NSAMPLES)).any()      # more hits than any nsample
        # the window over the occupied half: every row of it full (x = 0 .. 19); the one cut by the half's face: a few cells per row
        assert (c == rows * 20).any() and ((c > 0) & (c <= rows * 9)).any() and (c == 0).any()


@pytest.mark.parametrize("name,radius", R.CASE3)
def test_case3_windows_partly_and_wholly_outside_on_each_axis_and_side(oracle, name, radius):
    sc = R.SCENES[name]()
    for ranges in R.CASE3_RANGES:
        q = R.queries_outside(sc, ranges)
        assert (q[:, 0] >= 0).all() and (q[:, 0] < sc["batch"]).all()
        c = _counts(oracle, sc, ranges, radius, q)
        for a, (r, s) in enumerate(zip(ranges, sc["shape"])):
            v = q[:, 1 + a]
            low_part, low_out = (v - r < 0) & (v + r >= 0), v + r < 0
            high_part, high_out = (v + r >= s) & (v - r < s), v - r >= s
            for part, out in ((low_part, low_out), (high_part, high_out)):
                assert (c[part] > 0).any(), (ranges, a)
                assert out.any() and (c[out] == 0).all(), (ranges, a)


def test_case4_rows_start_at_every_bit_offset_and_straddle_words():
    offs, two = set(), False
    for r3 in R.WORDS_R3:
        sc = R.words(r3, "full")
        for ranges in R.CASE4_RANGES:
            o, t = R.row_starts(sc, R.queries_every_cell(sc), ranges[2])
            offs |= o
            two |= t
    assert offs == set(range(64)) and two
    # a 31-bit row that ends on the very last bit of the bitmap's last word, and one that ends inside it
    for r3, want in ((32, True), (31, False)):
        sc = R.words(r3, "full")
        cells = sc["batch"] * int(np.prod(sc["shape"]))
        assert (cells % 64 == 0) == want


def test_far_scene_has_hits_at_a_distance_equal_to_the_radius(oracle):
    sc = R.far()
    q = R.queries_far(sc)
    qxyz = R.centres(sc, q[:, 1:4])
    xyz = R.centres(sc, sc["cells"][:, 1:4])
    lut = np.full((1, *sc["shape"]), -1, np.int64)
    lut[tuple(sc["cells"].T)] = np.arange(len(sc["cells"]))
    line = R.centres(sc, np.stack([np.zeros(200, int), np.zeros(200, int), np.arange(sc["shape"][2] - 200, sc["shape"][2])], 1))[:, 0]
    for k in R.FAR_K:
        radius = R.far_radius(sc, line, k)
        r2 = np.float32(radius) * np.float32(radius)
        assert abs(radius - k * 0.1) < 1e-5
        # the outermost cells the ball reaches along x: same z, y, x +- k
        on_rim = 0
        for side in (-k, k):
            x = q[:, 3] + side
            ok = (x >= 0) & (x < sc["shape"][2])
            nb = lut[0, q[ok, 1], q[ok, 2], x[ok]]
            d2 = R.d2_fp32(xyz[nb[nb >= 0]], qxyz[ok][nb >= 0])
            on_rim += int((d2 == r2).sum())
            assert not (d2 == r2).all()                          # ... and next to them pairs the fp32 centres put just inside or outside
        assert on_rim > 100, on_rim
        c = _counts(oracle, sc, R.FAR_RANGE, radius, q, qxyz)
        assert (c > 0).any()


def test_pooling_reference_is_the_definition(oracle):
    rng = np.random.default_rng(0)
    n, m, ns, c, c2 = 40, 9, 5, 4, 6
    fin, xyz, new_xyz = rng.normal(size=(n, c)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(m, 3)).astype(np.float32)
    idx = rng.integers(0, n, (m, ns)).astype(np.int32)
    idx[3] = [-1, 0, 0, 0, 0]
    w_pos, b_pos = rng.normal(size=(3, c)).astype(np.float32), rng.normal(size=c).astype(np.float32)
    w_out, t_out = rng.normal(size=(c, c2)).astype(np.float32), rng.normal(size=c2).astype(np.float32)
    got, bound = R.pool_max(fin, xyz, new_xyz, idx, w_pos, b_pos)
    # the module's sequence: group (oracle.group_points), zero the empty balls, position MLP, add, ReLU, max over the samples
    one = np.array([n], np.int32), np.array([m], np.int32)
    safe = np.where(idx < 0, 0, idx)
    gf = oracle.group_points(fin, one[0], safe, one[1]).astype(np.float64)                  # [m, c, ns]
    gx = oracle.group_points(xyz, one[0], safe, one[1]).astype(np.float64) - new_xyz.astype(np.float64)[:, :, None]
    gf[3], gx[3] = 0, 0
    pos = np.einsum("mds,dc->mcs", gx, w_pos.astype(np.float64)) + b_pos.astype(np.float64)[None, :, None]
    want = np.maximum(gf + pos, 0).max(2)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    assert (bound[3] == 0).all() and (np.delete(bound, 3, 0) > 0).all() and bound.max() < 1e-5
    for relu in (0, 1):
        out, ob = R.pool_max_mlp(fin, xyz, new_xyz, idx, w_pos, b_pos, w_out, t_out, relu)
        w = want @ w_out.astype(np.float64) + t_out
        np.testing.assert_allclose(out, np.maximum(w, 0) if relu else w, rtol=0, atol=1e-13)
        assert (ob > 0).all() and (out == 0).any() == bool(relu)
    # fp32 evaluation in the kernel's order stays inside the bound (the bound is not vacuous: it is within 100x of the error)
    f32 = np.float32
    err = np.zeros_like(got)
    for i in range(m):
        if idx[i, 0] < 0:
            continue
        d = xyz[idx[i]] - new_xyz[i]
        p = ((d[:, 0:1] * w_pos[0] + d[:, 1:2] * w_pos[1]) + d[:, 2:3] * w_pos[2]) + b_pos
        assert p.dtype == f32
        err[i] = np.abs(np.maximum(fin[idx[i]] + p, f32(0)).max(0).astype(np.float64) - got[i])
    assert (err <= bound).all() and err.max() > bound.max() / 100
    # NaN and infinities as torch's ReLU and max treat them
    fin2 = fin.copy()
    fin2[idx[0, 1], 0], fin2[idx[1, 0], 1], fin2[idx[2, 2], 2] = np.nan, np.inf, -np.inf
    with np.errstate(invalid="ignore"):
        g2, _ = R.pool_max(fin2, xyz, new_xyz, idx, w_pos, b_pos)
    assert np.isnan(g2[0, 0]) and g2[1, 1] == np.inf and np.isfinite(g2[2, 2]) and g2[2, 2] >= 0


def test_grouping_reference_matches_the_oracle(oracle):
    rng = np.random.default_rng(1)
    fcnt, icnt = np.array([9, 0, 5], np.int32), np.array([4, 0, 3], np.int32)    # rows 7, 8: nobody points at them
    feat = rng.normal(size=(14, 3)).astype(np.float32)
    idx = np.concatenate([rng.integers(0, 7, (4, 5)), rng.integers(0, 5, (3, 5))]).astype(np.int32)
    got, rows = R.group_points(feat, fcnt, idx, icnt)
    np.testing.assert_array_equal(got, oracle.group_points(feat, fcnt, idx, icnt))
    assert rows[4:].min() >= 9
    go = rng.normal(size=got.shape).astype(np.float32)
    grad, bound = R.group_points_grad(go, rows, 14)
    want = np.zeros((14, 3))
    for pt in range(7):
        for s in range(5):
            want[rows[pt, s]] += go[pt, :, s].astype(np.float64)
    np.testing.assert_allclose(grad, want, rtol=0, atol=1e-14)
    untouched = np.setdiff1d(np.arange(14), rows)
    assert untouched.size and (grad[untouched] == 0).all() and (bound[untouched] == 0).all()
