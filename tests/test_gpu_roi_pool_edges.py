"""The voxel-query, fused pooling and grouping kernels of cpd_amd/csrc/roi_pool.hip at their edges.

Queries (cases 1 - 6): the four paths -- dense volume, bitmap index row-wise, bitmap index cell-wise (x range 16), index + cell
geometry -- against oracle.voxel_query on the scenes of tests/ref_roi_pool_edges.py, raw output, every slot, assert_array_equal:
sample counts beside and above 16, waves whose groups finish at different steps, windows partly and wholly outside the grid, window
rows at every bit offset of the bitmap, indexes in all three row orders, radii of 0 / exactly k cells / unlimited, NaN and infinite
query coordinates. tests/test_roi_pool_edges_ref.py asserts on the CPU that the scenes contain these edges. Every call goes to the
C entry point with 16 sentinel rows behind row m of `idx`; they must come back untouched.

Pooling (7, 8): cpd_voxel_pool_max / _mlp / _mlp_ranged against the float64 definition with a per-element bound counted from the
kernel source (ref_roi_pool_edges.N_POOL, n_mlp), and NaN / infinite features against torch's ReLU and max. Grouping (9) and
cpd_voxel2pinds (10): batch edges and rows outside the grid."""
import numpy as np
import pytest
import torch

import ref_index_edges as RI
import ref_roi_pool_edges as R

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A                 # what the rows behind an output hold before a call
GUARD_ROWS = 16
UNSUPPORTED = -4
PATHS = ("dense", "index", "grid")   # `index`: rows kernel up to 32-cell rows, cell-wise beyond; `grid` takes only the former


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Level:
    """A scene on the device in one of the three row orders of an index (tests/test_gpu_index_edges.py MODES): xyz from
    get_voxel_centers on the rows as the features have them, read back for the oracle; dense volume; site index."""

    def __init__(self, oracle, sc, mode="canonical", seed=0):
        from cpd_amd import ops, roi_pool
        self.sc, self.batch, self.shape = sc, sc["batch"], sc["shape"]
        canon = sc["cells"]
        n = len(canon)
        rmap = np.random.default_rng(seed + 2).permutation(n).astype(np.int32)
        if mode == "canonical":
            rows = canon
        else:                                                    # row rmap[rank] holds the site of that rank
            rows = np.empty_like(canon)
            rows[rmap] = canon
        self.rows = np.ascontiguousarray(rows)
        self.cells = up(self.rows)
        self.xyz = roi_pool.get_voxel_centers(self.cells[:, 1:4], sc["stride"], sc["voxel_size"], sc["pcr"]).contiguous()
        self.xyz_h = self.xyz.cpu().numpy()
        np.testing.assert_array_equal(self.xyz_h, R.centres(sc, self.rows[:, 1:4]))
        self.v2p_h = oracle.voxel2pinds(self.rows, self.batch, self.shape)
        self.v2p = roi_pool.generate_voxel2pinds(self.cells, self.batch, self.shape)
        np.testing.assert_array_equal(self.v2p.cpu().numpy(), self.v2p_h)
        if mode == "installed":                                  # canonical list + a caller's rank -> row map (flags 2)
            self.index = ops.SiteIndex.build(up(canon), self.batch, self.shape).set_order(up(rmap))
        else:                                                    # `own`: a list in arbitrary order, through the index's own map (flags 1)
            self.index = ops.SiteIndex.build(self.cells, self.batch, self.shape)
        self.grid = roi_pool.cell_geometry(sc["voxel_size"], sc["stride"], sc["pcr"])


def launch_query(path, lv, ranges, radius, ns, m, d_q, d_qxyz):
    """one C entry point on m queries -> raw idx [m, ns]; the 16 rows behind it must keep the pattern"""
    from cpd_amd import ops
    from cpd_amd._lib import check, lib, ptr, stream
    buf = torch.full((m + GUARD_ROWS, ns), PATTERN, dtype=torch.int32, device="cuda")
    buf[:m] = 0                                                  # the kernels count on the caller's zeros
    z, y, x = lv.shape
    zr, yr, xr = ranges
    n = lv.xyz.shape[0]
    with ops.launch_log() as log:
        if path == "dense":
            check(lib().cpd_voxel_query(m, z, y, x, ns, radius, zr, yr, xr, ptr(d_qxyz), ptr(lv.xyz), ptr(d_q), ptr(lv.v2p), ptr(buf), stream()),
                  "cpd_voxel_query")
            label = None
        elif path == "index":
            check(lib().cpd_voxel_query_index(m, lv.batch, z, y, x, ns, radius, zr, yr, xr, ptr(d_qxyz), ptr(lv.xyz), ptr(d_q), ptr(lv.index.buf), 0,
                                              n, ptr(buf), stream()), "cpd_voxel_query_index")
            label = "voxel_query_rows_kernel" if 2 * xr + 1 <= 32 else "voxel_query_kernel<IndexLookup>"
        else:
            check(lib().cpd_voxel_query_index_grid(m, lv.batch, z, y, x, ns, radius, zr, yr, xr, ptr(d_qxyz), ptr(d_q), ptr(lv.index.buf), n,
                                                   lv.grid[0], lv.grid[1], ptr(buf), stream()), "cpd_voxel_query_index_grid")
            label = "voxel_query_grid_kernel"
    if label is not None:
        assert log.counts == ({label: 1} if m > 0 else {}), log.counts
    out = buf.cpu().numpy()
    assert (out[m:] == PATTERN).all(), "%s wrote behind row m" % path
    return out[:m]


def check_paths(oracle, lv, ranges, radius, nsamples, q, qxyz, ms=None, paths=PATHS):
    """every path that takes `ranges`, every nsample, (every prefix m of the queries) against the oracle, slot for slot"""
    d_q, d_qxyz = up(q), up(qxyz)
    for ns in nsamples:
        want = oracle.voxel_query(ranges, radius, ns, lv.xyz_h, qxyz, q, lv.v2p_h)
        for path in paths:
            if path == "grid" and 2 * ranges[2] + 1 > 32:
                continue
            for m in (ms if ms is not None else [len(q)]):
                got = launch_query(path, lv, ranges, radius, ns, m, d_q, d_qxyz)
                np.testing.assert_array_equal(got, want[:m], err_msg="%s ranges %s nsample %d m %d" % (path, ranges, ns, m))
    return want


@pytest.fixture(scope="module")
def levels(oracle, hip):
    cache = {}

    def get(name, mode="canonical"):
        if (name, mode) not in cache:
            cache[name, mode] = Level(oracle, R.SCENES[name](), mode)
        return cache[name, mode]
    return get


# ------------------------------------------------------------------------------------------------ 1: sample counts
@pytest.mark.parametrize("ranges", R.RANGES, ids=str)
@pytest.mark.parametrize("name,radius", R.CASE1)
def test_1_sample_counts_beside_and_above_sixteen(oracle, levels, name, radius, ranges):
    lv = levels(name)
    q = R.queries_around(lv.sc, ranges)
    want = check_paths(oracle, lv, ranges, radius, R.NSAMPLES, q, R.centres(lv.sc, q[:, 1:4]))
    assert (want[:, 0] == -1).any() and (want[want[:, 0] == -1][:, 1:] == 0).all()           # the `-1, 0, 0, ...` rows
    assert ((want[:, 0] >= 0) & (want[:, -1] == want[:, 0])).any()                           # pre-filled slots (nsample 48)


# ------------------------------------------------------------------------------------------------ 2: ragged m
@pytest.mark.parametrize("ranges", ([1, 2, 15], [1, 1, 16]), ids=str)
def test_2_small_m_and_waves_whose_groups_finish_apart(oracle, levels, ranges):
    lv = levels("half")
    q = R.queries_ragged(lv.sc, 65)
    check_paths(oracle, lv, ranges, R.RADIUS_ALL, (5, 32), q, R.centres(lv.sc, q[:, 1:4]), ms=(0, 1, 15, 16, 17, 63, 65))


# ------------------------------------------------------------------------------------------------ 3: cells outside the grid
@pytest.mark.parametrize("ranges", R.CASE3_RANGES, ids=str)
@pytest.mark.parametrize("name,radius", R.CASE3)
def test_3_windows_partly_and_wholly_outside_the_grid(oracle, levels, name, radius, ranges):
    lv = levels(name)
    q = R.queries_outside(lv.sc, ranges)
    check_paths(oracle, lv, ranges, radius, (5, 16, 17), q, R.centres(lv.sc, q[:, 1:4]))


# ------------------------------------------------------------------------------------------------ 4: bitmap words
@pytest.mark.parametrize("pattern", ("full", "checker"))
@pytest.mark.parametrize("r3", R.WORDS_R3)
def test_4_window_rows_at_every_bit_offset(oracle, hip, r3, pattern):
    lv = Level(oracle, R.words(r3, pattern))
    q = R.queries_every_cell(lv.sc)
    qxyz = R.centres(lv.sc, q[:, 1:4])
    for ranges in R.CASE4_RANGES:
        for radius in (R.RADIUS_ALL, 2.05 * 0.4):               # the whole row, and a ball that cuts it (the grid kernel's xlo moves)
            check_paths(oracle, lv, ranges, radius, (16, 48), q, qxyz)


# ------------------------------------------------------------------------------------------------ 5: row order
@pytest.mark.parametrize("name", ("sparse", "checker"))
def test_5_indexes_in_every_row_order(oracle, hip, name):
    """flags[0] of the index buffer (site_index_layout.h): 1 -- the index's own map, identity for a canonical list and a real
    permutation for a shuffled one; 2 -- a map installed from outside; 0 -- after set_order(None), rank is row"""
    sc = R.SCENES[name]()
    q = R.queries_around(sc, [1, 1, 1])[::3]
    qxyz = R.centres(sc, q[:, 1:4])
    cases = (([1, 2, 15], 1.3), ([1, 1, 16], 2.5), ([2, 2, 2], 0.9))

    def flags(lv):
        return int(lv.index.buf[:4].view(torch.int32)[0])
    lvs = {mode: Level(oracle, sc, mode) for mode in ("canonical", "own", "installed")}
    for mode, want in (("canonical", 1), ("own", 1), ("installed", 2)):
        assert flags(lvs[mode]) == want
        assert (mode == "canonical") == np.array_equal(lvs[mode].rows, sc["cells"])
        for ranges, radius in cases:
            check_paths(oracle, lvs[mode], ranges, radius, (5, 17), q, qxyz)
    # the installed map dropped again: the same index now answers in canonical rows
    back = lvs["canonical"]
    back.index = lvs["installed"].index.set_order(None)
    assert flags(back) == 0
    for ranges, radius in cases:
        check_paths(oracle, back, ranges, radius, (5, 17), q, qxyz, paths=("index", "grid"))


# ------------------------------------------------------------------------------------------------ 6: radius and coordinate edges
def test_6_radius_zero_hits_the_centre_cell(oracle, levels):
    for name in ("checker", "sparse"):
        lv = levels(name)
        q = R.queries_every_cell(lv.sc)
        for ranges in ([1, 1, 1], [1, 2, 15], [1, 1, 16]):
            want = check_paths(oracle, lv, ranges, 0.0, (1, 5), q, R.centres(lv.sc, q[:, 1:4]))
            occupied = lv.v2p_h[tuple(q.T)]
            np.testing.assert_array_equal(want[:, 0], occupied)      # `not >`: exactly the query's own cell, where it is occupied


@pytest.mark.parametrize("k", R.FAR_K)
def test_6_radius_of_exactly_k_cells_far_from_the_origin(oracle, levels, k):
    lv = levels("far")
    q = R.queries_far(lv.sc)
    qxyz = R.centres(lv.sc, q[:, 1:4])
    radius = R.far_radius(lv.sc, qxyz[:200, 0], k)               # (the first 200 queries are one x line)
    assert (np.diff(q[:200, 3]) == 1).all()
    for ranges in (R.FAR_RANGE, [1, 1, 16]):
        check_paths(oracle, lv, ranges, radius, (16, 48), q, qxyz)
    check_paths(oracle, lv, R.FAR_RANGE, R.RADIUS_ALL, (48,), q, qxyz)                       # only the window limits the hits


@pytest.mark.parametrize("radius", (0.5, 1.3, R.RADIUS_ALL))
def test_6_nan_and_infinite_query_coordinates(oracle, levels, radius):
    """oracle: a NaN coordinate makes d2 NaN and `not >` takes every occupied cell of the window; an infinite one gives d2 = inf
    (or NaN beside a NaN / an opposite infinity) -- whatever the oracle answers is expected of every path"""
    lv = levels("checker")
    q = R.queries_around(lv.sc, [1, 1, 1])[::7].copy()
    qxyz = R.centres(lv.sc, q[:, 1:4])
    bad = [np.nan, np.inf, -np.inf]
    for i in range(0, len(q), 3):                                # every third query: one or two wild coordinates
        qxyz[i, (i // 3) % 3] = bad[(i // 9) % 3]
        if (i // 27) % 2:
            qxyz[i, (i // 3 + 1) % 3] = bad[(i // 54) % 3]
    for ranges in ([1, 1, 1], [2, 2, 2], [1, 2, 15], [1, 1, 16]):
        with np.errstate(invalid="ignore"):
            want = check_paths(oracle, lv, ranges, radius, (5, 32), q, qxyz)
        wild = ~np.isfinite(qxyz).all(1)
        assert (want[wild & np.isnan(qxyz).any(1), 0] >= 0).any() and (want[np.isinf(qxyz).any(1) & ~np.isnan(qxyz).any(1), 0] == -1).all()


# ------------------------------------------------------------------------------------------------ 7: pooling against float64
NS_POOL = (1, 5, 16, 32)
POOL_RANGE, POOL_RADIUS = [1, 2, 2], 1.3


class PoolCase:
    """Inputs of the pooling kernels on `sparse` for C channels: feature rows strided (ld = C + 3), the lowest layer's features
    shifted far below zero (a ball that holds only those pools to exactly 0), idx = the raw output of a real query per nsample
    (empty balls, pre-filled slots), all balls empty, and a hand-made idx that repeats its first entry in later slots."""

    def __init__(self, oracle, lv, c):
        rng = np.random.default_rng(100 + c)
        self.c, self.lv = c, lv
        self.p = 256 // c
        self.m_max = 8 * self.p + 1
        n = lv.xyz_h.shape[0]
        fin = rng.normal(size=(n, c + 3)).astype(np.float32)
        fin[lv.rows[:, 1] == 0, :c] -= 50.0
        self.fin_h, self.fin = fin, up(fin)
        Z, Y, X = lv.shape
        q = np.stack([rng.integers(0, 2, self.m_max), rng.integers(0, Z, self.m_max), rng.integers(0, Y, self.m_max),
                      rng.integers(0, X, self.m_max)], 1).astype(np.int32)
        q[1::4, 1] = -1                                                          # only the lowest layer in reach: pools to exactly 0
        q[2::4, 1] = -2                                                          # nothing in reach: an empty ball
        q[0] = [0] + lv.rows[lv.rows[:, 0] == 0][5, 1:].tolist()                 # m = 1: a ball that is not empty
        self.q = np.ascontiguousarray(q)
        self.qxyz = (R.centres(lv.sc, q[:, 1:4]) + rng.uniform(-0.2, 0.2, (self.m_max, 3)).astype(np.float32)).astype(np.float32)
        self.w_pos, self.b_pos = rng.normal(size=(3, c)).astype(np.float32), rng.normal(size=c).astype(np.float32)
        self.w_out, self.t_out = (rng.normal(size=(c, 2 * c + 1)) * 0.3).astype(np.float32), rng.normal(size=2 * c + 1).astype(np.float32)
        self.d = dict(xyz=lv.xyz, qxyz=up(self.qxyz), w_pos=up(self.w_pos), b_pos=up(self.b_pos))
        self.idx, self.ref = {}, {}
        d_q = up(self.q)
        for ns in NS_POOL:
            self.idx["query", ns] = launch_query("index", lv, POOL_RANGE, POOL_RADIUS, ns, self.m_max, d_q, self.d["qxyz"])
        e = np.zeros((self.m_max, 5), np.int32)
        e[:, 0] = -1
        self.idx["empty", 5] = e
        h = rng.integers(0, n, (self.m_max, 16)).astype(np.int32)
        h[:, [3, 7, 15]] = h[:, :1]                                              # the kernel's `j == j0` skip, between real entries
        h[::5, 0] = -1
        self.idx["repeats", 16] = h
        for key, idx in self.idx.items():
            self.ref[key] = R.pool_max(fin[:, :c], lv.xyz_h, self.qxyz, idx, self.w_pos, self.b_pos)
        i16, i5 = self.idx["query", 16], self.idx["query", 5]
        assert (i16[:, 0] == -1).any() and ((i16[:, 0] >= 0) & (i16[:, -1] == i16[:, 0])).any()      # empty balls, pre-filled slots
        assert ((i5[:, 0] >= 0) & (i5[:, -1] != i5[:, 0])).any()                 # ... and balls that fill every slot
        pooled = self.ref["query", 16][0]
        assert ((pooled == 0).all(1) & (i16[:, 0] >= 0)).any()                   # whole rows cut to 0 by the ReLU


def _ratio(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    assert (err[bound == 0] == 0).all(), what
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert r <= 1.0, "%s: error / bound = %.3f" % (what, r)
    return r


def _wide(m, width):
    return torch.full((m + GUARD_ROWS, width), -7.0, device="cuda")


@pytest.mark.parametrize("c", (16, 24, 32, 64, 128))
def test_7_pool_max_against_float64(oracle, levels, c):
    from cpd_amd._lib import check, lib, ptr, stream
    pc = PoolCase(oracle, levels("sparse"), c)
    worst = 0.0
    for (kind, ns), idx in pc.idx.items():
        want, bound = pc.ref[kind, ns]
        d_idx = up(idx)
        for m in (1, 8 * pc.p - 1, 8 * pc.p, 8 * pc.p + 1):
            wide = _wide(m, c + 9)
            check(lib().cpd_voxel_pool_max(m, c, ns, ptr(pc.fin), pc.fin.stride(0), ptr(pc.d["xyz"]), ptr(pc.d["qxyz"]), ptr(d_idx), ptr(pc.d["w_pos"]),
                                           ptr(pc.d["b_pos"]), wide[:, 4:].data_ptr(), wide.stride(0), stream()), "cpd_voxel_pool_max")
            out = wide.cpu().numpy()
            assert (out[:, :4] == -7).all() and (out[:, 4 + c:] == -7).all() and (out[m:] == -7).all()
            worst = max(worst, _ratio(out[:m, 4:4 + c], want[:m], bound[:m], "pool_max C %d %s nsample %d m %d" % (c, kind, ns, m)))
            zero = (want[:m] == 0).all(1)
            assert (out[:m, 4:4 + c][zero] == 0).all()
    print("voxel_pool_max C = %d: largest error / bound = %.3f" % (c, worst))


@pytest.mark.parametrize("c", (16, 32, 64))
def test_7_pool_max_mlp_and_ranged_against_float64(oracle, levels, c):
    from cpd_amd import ops
    from cpd_amd._lib import check, lib, ptr, stream
    pc = PoolCase(oracle, levels("sparse"), c)
    worst = 0.0
    seeded = int(np.float32(1e30).view(np.int32))
    for c2 in (1, c - 1, c, c + 1, 2 * c):
        w_out, t_out = np.ascontiguousarray(pc.w_out[:, :c2]), pc.t_out[:c2]
        d_w, d_t = up(w_out), up(t_out)
        for (kind, ns), idx in pc.idx.items():
            pooled, pb = pc.ref[kind, ns]
            d_idx = up(idx)
            for relu in (0, 1):
                want, bound = R.mlp(pooled, pb, w_out, t_out, relu)
                for m in (1, 8 * pc.p - 1, 8 * pc.p, 8 * pc.p + 1):
                    what = "pool_max_mlp C %d c2 %d relu %d %s nsample %d m %d" % (c, c2, relu, kind, ns, m)
                    args = (m, c, ns, ptr(pc.fin), pc.fin.stride(0), ptr(pc.d["xyz"]), ptr(pc.d["qxyz"]), ptr(d_idx), ptr(pc.d["w_pos"]),
                            ptr(pc.d["b_pos"]), ptr(d_w), ptr(d_t), c2, relu)
                    wide, wide_r = _wide(m, c2 + 9), _wide(m, c2 + 9)
                    blocks = ops.absmax_blocks(2, "cuda")
                    blocks[1, 0] = seeded
                    with ops.launch_log() as log:
                        check(lib().cpd_voxel_pool_max_mlp(*args, wide[:, 4:].data_ptr(), wide.stride(0), stream()), "cpd_voxel_pool_max_mlp")
                        check(lib().cpd_voxel_pool_max_mlp_ranged(*args, wide_r[:, 4:].data_ptr(), wide_r.stride(0), ptr(blocks[0]), stream()), "ranged")
                        check(lib().cpd_voxel_pool_max_mlp_ranged(*args, wide_r[:, 4:].data_ptr(), wide_r.stride(0), ptr(blocks[1]), stream()), "ranged")
                    assert log.counts == {"voxel_pool_max_mlp_kernel": 3}
                    out, out_r = wide.cpu().numpy(), wide_r.cpu().numpy()
                    np.testing.assert_array_equal(out_r, out)
                    assert (out[:, :4] == -7).all() and (out[:, 4 + c2:] == -7).all() and (out[m:] == -7).all(), what
                    blk = out[:m, 4:4 + c2]
                    worst = max(worst, _ratio(blk, want[:m], bound[:m], what))
                    # the absmax block: the bits of max |value written|, from the kernel's own output; a larger word is not lowered
                    words = blocks.cpu().numpy()
                    assert words[0].max() == int(np.abs(blk).max().view(np.int32)), what
                    assert words[1, 0] == seeded and words[1].max() == seeded, what
    print("voxel_pool_max_mlp C = %d: largest error / bound = %.3f" % (c, worst))


def test_7_unsupported_shapes_are_refused_and_write_nothing(oracle, levels):
    from cpd_amd import ops
    from cpd_amd._lib import lib, ptr, stream
    pc = PoolCase(oracle, levels("sparse"), 16)
    ns, m = 5, 20
    d_idx = up(pc.idx["query", ns])
    wide, block = _wide(m, 128), ops.absmax_blocks(1, "cuda")
    fin48 = torch.zeros((pc.fin.shape[0], 48), device="cuda")
    w48, t = torch.zeros((48, 97), device="cuda"), torch.zeros(97, device="cuda")
    for c, c2, fin in ((16, 33, pc.fin), (48, 16, fin48), (48, 97, fin48)):
        args = (m, c, ns, ptr(fin), fin.stride(0), ptr(pc.d["xyz"]), ptr(pc.d["qxyz"]), ptr(d_idx), ptr(w48), ptr(t), ptr(w48), ptr(t), c2, 1)
        with ops.launch_log() as log:
            assert lib().cpd_voxel_pool_max_mlp(*args, ptr(wide), wide.stride(0), stream()) == UNSUPPORTED
            assert lib().cpd_voxel_pool_max_mlp_ranged(*args, ptr(wide), wide.stride(0), ptr(block), stream()) == UNSUPPORTED
        assert log.counts == {}
    assert bool((wide == -7).all()) and bool((block == 0).all())


# ------------------------------------------------------------------------------------------------ 8: NaN and infinity
def test_8_nan_and_infinite_features_come_out_as_torch_gives_them(oracle, levels):
    """Expected: voxel_query_and_grouping, then the module's torch sequence (position MLP, add, ReLU, max; output MLP) -- a NaN
    wherever a NaN enters a ball, +inf kept, -inf cut by the ReLU. Where torch's value is finite the float64 reference and its bound
    hold as in case 7."""
    from cpd_amd import ops, roi_pool
    from cpd_amd._lib import check, lib, ptr, stream
    lv = levels("sparse")
    c, c2, ns = 16, 24, 16
    pc = PoolCase(oracle, lv, c)
    order = np.argsort(pc.q[:, 0], kind="stable")
    q, qxyz = np.ascontiguousarray(pc.q[order]), np.ascontiguousarray(pc.qxyz[order])
    m = len(q)
    idx0 = oracle.voxel_query(POOL_RANGE, POOL_RADIUS, ns, lv.xyz_h, qxyz, q, lv.v2p_h)
    hit = idx0[idx0[:, 0] >= 0]
    fin = pc.fin_h[:, :c].copy()
    fin[hit[0, 0], 2:5] = np.nan
    fin[hit[len(hit) // 2, 1], 0:3] = np.inf
    fin[hit[-1, 0], 5:9] = -np.inf
    k_nan = int(np.flatnonzero(idx0[:, 0] >= 0)[3])
    qxyz[k_nan, 1] = np.nan                                      # the query: every occupied cell of its window; the pooling: NaN offsets
    d_fin, d_q, d_qxyz = up(fin), up(q), up(qxyz)
    with np.errstate(invalid="ignore"):
        idx = launch_query("index", lv, POOL_RANGE, POOL_RADIUS, ns, m, d_q, d_qxyz)
        np.testing.assert_array_equal(idx, oracle.voxel_query(POOL_RANGE, POOL_RADIUS, ns, lv.xyz_h, qxyz, q, lv.v2p_h))
    cnt = torch.from_numpy(np.bincount(lv.rows[:, 0], minlength=2).astype(np.int32)).cuda()
    qcnt = torch.from_numpy(np.bincount(q[:, 0], minlength=2).astype(np.int32)).cuda()
    gf, gx, empty = roi_pool.voxel_query_and_grouping(POOL_RANGE, POOL_RADIUS, ns, d_q, lv.xyz, cnt, d_qxyz, qcnt, d_fin, index=lv.index)
    np.testing.assert_array_equal(empty.cpu().numpy(), idx[:, 0] == -1)
    w_pos, b_pos = pc.d["w_pos"], pc.d["b_pos"]
    w_out, t_out = np.ascontiguousarray(pc.w_out[:, :c2]), pc.t_out[:c2]
    d_w, d_t = up(w_out), up(t_out)
    rel = gx - d_qxyz[:, :, None]
    rel[empty], gf[empty] = 0, 0
    pos = (rel[:, :, None, :] * w_pos[None, :, :, None]).sum(1) + b_pos[None, :, None]
    pooled_t = torch.relu(gf + pos).max(dim=2).values
    out_t = {0: pooled_t @ d_w + d_t, 1: torch.relu(pooled_t @ d_w + d_t)}
    assert bool(torch.isnan(pooled_t).any()) and bool(torch.isinf(pooled_t).any()) and bool(torch.isnan(pooled_t[k_nan]).all())

    def same(got, want_t, want64, bound, what):
        want_t = want_t.cpu().numpy()
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want_t), err_msg=what)
        inf = np.isinf(want_t)
        np.testing.assert_array_equal(got[inf], want_t[inf], err_msg=what)
        np.testing.assert_array_equal(np.isnan(want64), np.isnan(want_t), err_msg=what)
        fin_ = np.isfinite(want_t) & np.isfinite(bound)
        assert fin_.sum() > fin_.size // 2 and (np.abs(got[fin_] - want64[fin_]) <= bound[fin_]).all(), what

    d_idx = up(idx)
    with np.errstate(invalid="ignore", over="ignore"):
        want64, pb = R.pool_max(fin, lv.xyz_h, qxyz, idx, pc.w_pos, pc.b_pos)
        got = roi_pool.voxel_pool_max(d_fin, lv.xyz, d_qxyz, d_idx, w_pos, b_pos).cpu().numpy()
        same(got, pooled_t, want64, pb, "voxel_pool_max")
        for relu in (0, 1):
            o64, ob = R.mlp(want64, pb, w_out, t_out, relu)
            out = torch.empty((m, c2), device="cuda")
            block = ops.absmax_blocks(1, "cuda")
            check(lib().cpd_voxel_pool_max_mlp_ranged(m, c, ns, ptr(d_fin), c, ptr(lv.xyz), ptr(d_qxyz), ptr(d_idx), ptr(w_pos), ptr(b_pos), ptr(d_w),
                                                      ptr(d_t), c2, relu, ptr(out), c2, ptr(block), stream()), "cpd_voxel_pool_max_mlp_ranged")
            same(out.cpu().numpy(), out_t[relu], o64, ob, "voxel_pool_max_mlp relu %d" % relu)
            # the range guard downstream reads this word: a NaN's magnitude bits compare above every finite word and above infinity
            assert int(block.max()) > 0x7f800000
            assert int(block.max()) == int((out.view(torch.int32) & 0x7fffffff).max())


# ------------------------------------------------------------------------------------------------ 9: grouping at batch edges
GROUP_CASES = [([37], [11], 5, 3), ([20, 0, 9], [5, 0, 7], 5, 3), ([6, 4, 0, 8], [3, 0, 0, 6], 5, 3), ([6, 4, 8, 0], [3, 0, 6, 0], 5, 3),
               ([50, 0, 30], [40, 0, 31], 7, 5)]


@pytest.mark.parametrize("fcnt,icnt,c,ns", GROUP_CASES, ids=str)
def test_9_group_points_and_its_gradient_at_batch_edges(oracle, hip, fcnt, icnt, c, ns):
    from cpd_amd import ops, roi_pool
    from cpd_amd._lib import check, lib, ptr, stream
    rng = np.random.default_rng(sum(fcnt) + len(fcnt))
    fcnt, icnt = np.array(fcnt, np.int32), np.array(icnt, np.int32)
    n, m = int(fcnt.sum()), int(icnt.sum())
    assert (m * c * ns) % 256 != 0
    feat = rng.normal(size=(n, c)).astype(np.float32)
    # many slots on one row: half of every sample's slots point at its rows 0 and 1, the sample's last row is never named
    idx = np.concatenate([np.where(rng.random((k, ns)) < 0.5, rng.integers(0, 2, (k, ns)), rng.integers(0, f - 1, (k, ns)))
                          for f, k in zip(fcnt, icnt) if k]).astype(np.int32)
    want, rows = R.group_points(feat, fcnt, idx, icnt)
    np.testing.assert_array_equal(want, oracle.group_points(feat, fcnt, idx, icnt))
    d_fcnt, d_icnt, d_idx = up(fcnt), up(icnt), up(idx)
    with ops.launch_log() as log:
        got = roi_pool.grouping_operation(up(feat), d_fcnt, d_idx, d_icnt)
    assert log.counts == {"group_points_kernel": 1}
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    go = rng.normal(size=(m, c, ns)).astype(np.float32)
    grad = torch.full((n + GUARD_ROWS, c), -7.0, device="cuda")
    with ops.launch_log() as log:
        check(lib().cpd_group_points_grad(len(fcnt), m, c, ns, n, ptr(up(go)), ptr(d_fcnt), ptr(d_idx), ptr(d_icnt), ptr(grad), stream()),
              "cpd_group_points_grad")
    assert log.counts == {"group_points_grad_kernel": 1}
    grad = grad.cpu().numpy()
    assert (grad[n:] == -7).all()
    want_g, bound = R.group_points_grad(go, rows, n)
    assert (np.abs(grad[:n] - want_g) <= bound).all()
    nobody = np.setdiff1d(np.arange(n), rows)
    assert nobody.size >= (fcnt > 0).sum() and (grad[nobody] == 0).all()
    assert np.bincount(rows.reshape(-1)).max() >= 4


# ------------------------------------------------------------------------------------------------ 10: voxel2pinds, rows outside the grid
def test_10_voxel2pinds_ignores_rows_outside_the_grid(hip):
    from cpd_amd import roi_pool
    batch, shape = 2, [3, 4, 33]
    rng = np.random.default_rng(7)
    inside = RI.canonical(np.stack([rng.integers(0, batch, 150)] + [rng.integers(0, s, 150) for s in shape], 1), batch, shape)
    inside = np.unique(inside, axis=0)
    outside = np.array([[-1, 0, 0, 0], [batch, 0, 0, 0], [0, shape[0], 1, 1], [1, -1, 2, 2], [0, 1, shape[1], 3], [1, 2, -1, 4],
                        [0, 0, 0, shape[2]], [1, 2, 3, -1], [-5, -5, -5, -5], [1000, 1000, 1000, 1000]], np.int32)
    rows = np.concatenate([inside, outside]).astype(np.int32)
    rows = rows[rng.permutation(len(rows))]
    got = roi_pool.generate_voxel2pinds(up(rows), batch, shape).cpu().numpy()
    want = RI.lookup(rows, batch, shape)
    np.testing.assert_array_equal(got, want.astype(np.int32))
    assert (want >= 0).sum() == len(inside)
