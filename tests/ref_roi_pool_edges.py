"""Scenes, query sets and plain numpy references (no torch, no GPU) for the edge tests of cpd_amd/csrc/roi_pool.hip: the voxel
queries, the fused pooling kernels and the grouping kernels. tests/test_gpu_roi_pool_edges.py runs the HIP kernels on them;
tests/test_roi_pool_edges_ref.py checks on the CPU, with the C oracle, that every scene really contains the edge it is named for
and that the float64 pooling reference is the module's definition.

A scene is a dict: batch, shape [Z, Y, X], cells int32 [n, 4] (b, z, y, x) in canonical order, and the geometry
(voxel_size, stride, pcr) from which get_voxel_centers (common_utils.py:66-82) makes the voxels' xyz -- three fp32 operations per
axis, restated by `centres`. Expected NEIGHBOURS never come from this file: they are the oracle's."""
import itertools

import numpy as np

U = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest)


# ------------------------------------------------------------------------------------------------ scenes
def _scene(batch, shape, occ, voxel_size=(0.1, 0.1, 0.15), stride=4, origin=(-3.0, -2.0, -1.0)):
    cells = np.argwhere(occ).astype(np.int32)                    # argwhere order IS canonical (b, z, y, x) order
    assert occ.shape == (batch, *shape)
    return dict(batch=batch, shape=list(shape), cells=np.ascontiguousarray(cells), voxel_size=list(voxel_size), stride=stride,
                pcr=list(origin) + [0.0, 0.0, 0.0])


def _grid(batch, shape):
    return np.indices((batch, *shape))


SHAPE = (5, 9, 40)


def dense():
    return _scene(2, SHAPE, np.ones((2, *SHAPE), bool))


def sparse():
    """about one cell in ten"""
    return _scene(2, SHAPE, np.random.default_rng(11).random((2, *SHAPE)) < 0.1)


def checker():
    b, z, y, x = _grid(2, SHAPE)
    return _scene(2, SHAPE, (z + y + x) % 2 == 0)


def half():
    """every cell with x < 20, nothing beyond: a full window and an empty one a few cells apart"""
    b, z, y, x = _grid(2, SHAPE)
    return _scene(2, SHAPE, x < 20)


WORDS_R3 = (31, 32, 33, 64, 65)


def words(r3, pattern):
    """[2, 3, r3] x batch 2: 12 rows of r3 cells back to back in the bitmap, `full` or `checker`"""
    shape = (2, 3, r3)
    b, z, y, x = _grid(2, shape)
    return _scene(2, shape, np.ones((2, *shape), bool) if pattern == "full" else (b + z + y + x) % 2 == 0)


FAR_SHAPE = (3, 5, 1504)


def far():
    """the Waymo range's last cells at stride 1: 1504 cells of 0.1 m from -75.2 m, about half occupied"""
    return _scene(1, FAR_SHAPE, np.random.default_rng(12).random((1, *FAR_SHAPE)) < 0.5, stride=1, origin=(-75.2, -75.2, -2.0))


def cell_size(sc):
    return (np.float32(sc["voxel_size"]) * np.float32(sc["stride"])).astype(np.float32)


def centres(sc, zyx):
    """get_voxel_centers for int cells [n, 3] (z, y, x) -> fp32 [n, 3] (x, y, z); also the `natural centre` of a cell outside the grid"""
    c = np.asarray(zyx)[:, [2, 1, 0]].astype(np.float32)
    return np.ascontiguousarray((c + np.float32(0.5)) * cell_size(sc) + np.float32(sc["pcr"][0:3]))


# ------------------------------------------------------------------------------------------------ query sets
def _sorted_by_batch(q):
    return np.ascontiguousarray(q[np.argsort(q[:, 0], kind="stable")].astype(np.int32))


def queries_around(sc, ranges):
    """every cell of the grid AND of a margin of range + 1 cells around it, in both samples: all window sizes the grid's faces,
    edges and corners can cut, down to none"""
    axes = [np.arange(-r - 1, s + r + 1) for r, s in zip(ranges, sc["shape"])]
    q = np.array(list(itertools.product(range(sc["batch"]), *axes)), np.int32)
    return _sorted_by_batch(q)


def queries_every_cell(sc):
    q = np.array(list(itertools.product(range(sc["batch"]), *[range(s) for s in sc["shape"]])), np.int32)
    return _sorted_by_batch(q)


def outside_values(size, rng_, r):
    """per axis: far outside, one beyond the window's reach, just within it, the faces, and two cells inside the grid"""
    return [-1000, -r - 1, -r, -1, 0, size - 1, size, size - 1 + r, size + r, 1000] + sorted(rng_.integers(1, size - 1, 2).tolist())


def queries_outside(sc, ranges, seed=3):
    rng_ = np.random.default_rng(seed)
    vals = [outside_values(s, rng_, r) for s, r in zip(sc["shape"], ranges)]
    q = np.array(list(itertools.product(*vals)), np.int64)
    q = np.concatenate([(np.arange(len(q)) % sc["batch"])[:, None], q], 1)           # the batch index stays valid
    return _sorted_by_batch(q)


def queries_ragged(sc, m):
    """m queries on `half` that cycle full window / empty window / window cut by the occupied half's face / empty, so that the four
    16-lane groups of a wave finish at different steps"""
    z, y = sc["shape"][0] // 2, sc["shape"][1] // 2
    cyc = [5, 37, 27, 38, 4, 36]
    q = np.array([[0, z, y, cyc[i % len(cyc)]] for i in range(m)], np.int32).reshape(-1, 4)
    return np.ascontiguousarray(q)


def queries_far(sc, last=200):
    """every cell of the last `last` x cells"""
    Z, Y, X = sc["shape"]
    q = np.array(list(itertools.product([0], range(Z), range(Y), range(X - last, X))), np.int32)
    return np.ascontiguousarray(q)


def far_radius(sc, xyz_centres_x, k):
    """`k cells` as the grid itself has them far from the origin: the fp32 difference of two x centres k cells apart that occurs
    most often among the last cells -- a query on a centre then has neighbours at a distance EQUAL to the radius in fp32"""
    d = (xyz_centres_x[k:] - xyz_centres_x[:-k]).astype(np.float32)
    vals, cnt = np.unique(d, return_counts=True)
    return float(vals[np.argmax(cnt)])


def d2_fp32(xyz, q):
    """the reference's distance test value (voxel_query_gpu.cu:58-60), fp32 operation for operation, for paired rows"""
    a = (xyz[:, 0] - q[:, 0]) * (xyz[:, 0] - q[:, 0])
    b = (xyz[:, 1] - q[:, 1]) * (xyz[:, 1] - q[:, 1])
    c = (xyz[:, 2] - q[:, 2]) * (xyz[:, 2] - q[:, 2])
    return (a + b) + c


def hit_counts(idx_big):
    """number of neighbours per query from a raw query output whose nsample exceeds every count: hits are distinct rows, the slots
    behind them repeat the first"""
    first = idx_big[:, :1]
    return np.where(first[:, 0] < 0, 0, 1 + (idx_big[:, 1:] != first).sum(1))


def row_starts(sc, q, xr):
    """bit offset (key & 63) of the first cell of every in-grid window row the rows kernel reads, and whether it needs two words"""
    Z, Y, X = sc["shape"]
    offs, two = set(), False
    for b, cz, cy, cx in q.tolist():
        x0, x1 = max(cx - xr, 0), min(cx + xr, X - 1)
        if x1 < x0:
            continue
        for z in range(max(cz - 1, 0), min(cz + 1, Z - 1) + 1):
            for y in range(max(cy - 1, 0), min(cy + 1, Y - 1) + 1):
                key = ((b * Z + z) * Y + y) * X + x0
                offs.add(key & 63)
                two |= (key & 63) + (x1 - x0 + 1) > 64
    return offs, two


# ------------------------------------------------------------------------------------------------ pooling, float64
# fp32 roundings on the longest path of one pooled element, from voxel_pool_max(_mlp)_kernel:
#   dx = xyz - new_xyz (1), dx * w (2), (dx w0 + dy w1) (3), + dz w2 (4), + b0 (5), fin + pos (6); ReLU and max round nothing
N_POOL = 6


def n_mlp(c):
    """... and of one output element of the MLP: the product p[0] * w[0] (1; adding it to the zero accumulator is exact), C - 1
    additions of the other products, + t_out: C + 1"""
    return c + 1


def pool_max(fin, xyz, new_xyz, idx, w_pos, b_pos):
    """out[m, c] = max_s relu(fin[j, c] + (xyz[j] - new_xyz[m]) . w_pos[:, c] + b_pos[c]), j = idx[m, s]; relu(b_pos) for an empty ball
    (idx[m, 0] < 0). float64 from the fp32 inputs. -> (out, bound): bound = N_POOL * 2^-24 * the largest sum of |terms| of a sample.
    NaN and infinities go through np.maximum like torch's ReLU and max (a NaN stays)."""
    fin, xyz, new_xyz, w_pos, b_pos = (np.asarray(a, np.float64) for a in (fin, xyz, new_xyz, w_pos, b_pos))
    m, ns = idx.shape
    c = w_pos.shape[1]
    out, bound = np.empty((m, c)), np.empty((m, c))
    for i in range(m):
        if idx[i, 0] < 0:
            out[i] = np.maximum(b_pos, 0.0)
            bound[i] = 0.0                                      # a copy of b_pos or 0: exact
            continue
        j = idx[i]
        d = xyz[j] - new_xyz[i]                                 # [ns, 3]
        terms = d[:, :, None] * w_pos[None]                     # [ns, 3, c]
        v = fin[j][:, :c] + terms.sum(1) + b_pos
        out[i] = _relu_max(v)
        bound[i] = N_POOL * U * (np.abs(fin[j][:, :c]) + np.abs(terms).sum(1) + np.abs(b_pos)).max(0)
    return out, bound


def _relu_max(v):
    return np.maximum(v, 0.0).max(0)                            # np.maximum and ndarray.max both keep a NaN, like torch


def mlp(pooled, pooled_bound, w_out, t_out, relu):
    """the output MLP on a pooled [m, C] block: pooled @ w_out + t_out, ReLU when `relu`. -> (out, bound): the MLP's own
    n_mlp(C) * 2^-24 * (|pooled| @ |w_out| + |t_out|) plus the pooled bound carried through |w_out|."""
    w_out, t_out = np.asarray(w_out, np.float64), np.asarray(t_out, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = pooled @ w_out + t_out
        bound = n_mlp(w_out.shape[0]) * U * (np.abs(pooled) @ np.abs(w_out) + np.abs(t_out)) + pooled_bound @ np.abs(w_out)
    return (np.maximum(out, 0.0) if relu else out), bound


def pool_max_mlp(fin, xyz, new_xyz, idx, w_pos, b_pos, w_out, t_out, relu):
    return mlp(*pool_max(fin, xyz, new_xyz, idx, w_pos, b_pos), w_out, t_out, relu)


def group_points(feat, fcnt, idx, icnt):
    """out[pt, c, s] = feat[start(sample of pt) + idx[pt, s], c] by fancy indexing"""
    fstart = np.concatenate([[0], np.cumsum(fcnt)[:-1]])
    sample = np.repeat(np.arange(len(icnt)), icnt)
    rows = fstart[sample][:, None] + idx                         # [m, ns]
    return feat[rows].transpose(0, 2, 1), rows


def group_points_grad(grad_out, rows, n):
    """float64 scatter-add of grad_out [m, c, ns] to the rows -> (grad [n, c], bound [n, c]): the atomics' order is free, so a row's
    sum of k addends is within k * 2^-24 * sum |addend| of the exact one"""
    m, c, ns = grad_out.shape
    g = np.asarray(grad_out, np.float64).transpose(0, 2, 1).reshape(-1, c)
    grad, absum, cnt = np.zeros((n, c)), np.zeros((n, c)), np.zeros(n)
    np.add.at(grad, rows.reshape(-1), g)
    np.add.at(absum, rows.reshape(-1), np.abs(g))
    np.add.at(cnt, rows.reshape(-1), 1)
    return grad, cnt[:, None] * U * absum


# ------------------------------------------------------------------------------------------------ the cases both test files share
SCENES = dict(dense=dense, sparse=sparse, checker=checker, half=half, far=far)
NSAMPLES = (1, 5, 16, 17, 32, 48)
RANGES = ([1, 1, 1], [2, 2, 2], [1, 2, 15], [1, 1, 16])      # x range 16: a 33-cell row, the index takes the cell-wise kernel
RADIUS_ALL = 1.0e4                                            # only the window limits the hits
CASE1 = [("dense", RADIUS_ALL), ("sparse", 1.3)]
CASE3 = [("checker", RADIUS_ALL), ("sparse", 1.3)]
CASE3_RANGES = ([2, 2, 2], [1, 2, 15], [1, 1, 16])
CASE4_RANGES = ([1, 1, 15], [1, 1, 7])
FAR_RANGE, FAR_K = [1, 2, 4], (1, 3)
