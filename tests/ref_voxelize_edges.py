"""Scenes (plain numpy, no torch, no GPU) for the edge tests of cpd_amd/csrc/voxelize.hip's first-appearance voxelizer, which serves
cpd_voxelize (one frame) and cpd_voxelize_batch* alike. tests/test_gpu_voxelize_edges.py runs the HIP kernels on them, one frame at a
time through both entry points; tests/test_voxelize_edges_ref.py checks on the CPU, with the C oracle, that every scene really
contains the edge it is named for.

A scene is a dict: points f32 [n, c], voxel_size, point_cloud_range, P (max points per voxel), max_voxels. Expected voxels never
come from this file: they are the oracle's. `cell_keys` restates the cell of a point only to COUNT what a scene holds."""
import numpy as np

GRID = dict(voxel_size=[1.0, 1.0, 1.0], point_cloud_range=[0.0, 0.0, 0.0, 8.0, 8.0, 4.0])       # 8 x 8 x 4 = 256 cells
WAYMO = dict(voxel_size=[0.1, 0.1, 0.15], point_cloud_range=[-75.2, -75.2, -2.0, 75.2, 75.2, 4.0])   # 1504 x 1504 x 40 = 9.05e7 cells
WAVE, BLOCK = 64, 256                # lanes of a wave, threads of a block in the point kernels


def grid_zyx(geo):
    vs, rg = np.float32(geo["voxel_size"]), np.float32(geo["point_cloud_range"])
    return np.round((rg[3:] - rg[:3]) / vs).astype(np.int64)[::-1]


def cell_keys(points, geo):
    """(z * Y + y) * X + x of every point, -1 outside the range (NaN and infinities included): fp32 floor((p - lo) / vs)"""
    vs, rg = np.float32(geo["voxel_size"]), np.float32(geo["point_cloud_range"])
    g = grid_zyx(geo)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((points[:, :3].astype(np.float32) - rg[:3]) / vs)[:, ::-1]              # z, y, x
        ok = np.all((c >= 0) & (c < g), axis=1)                                              # (a NaN compares false)
    ci = np.where(ok[:, None], c, 0).astype(np.int64)
    return np.where(ok, (ci[:, 0] * g[1] + ci[:, 1]) * g[2] + ci[:, 2], -1)


def _scene(points, geo=GRID, P=5, max_voxels=1000):
    return dict(points=np.ascontiguousarray(points, np.float32), P=P, max_voxels=max_voxels, **geo)


def _in_cells(rng, keys, geo, c):
    """one point somewhere inside each of the given cells, features in [0, 1)"""
    g = grid_zyx(geo)
    vs, rg = np.float64(geo["voxel_size"]), np.float64(geo["point_cloud_range"])
    keys = np.asarray(keys, np.int64)
    zyx = np.stack([keys // (g[1] * g[2]), keys // g[2] % g[1], keys % g[2]], 1)
    pts = np.empty((len(keys), c), np.float32)
    pts[:, :3] = rg[:3] + (zyx[:, ::-1] + rng.uniform(0.2, 0.8, (len(keys), 3))) * vs
    pts[:, 3:] = rng.uniform(0, 1, (len(keys), c - 3))
    return pts


# invalid xyz as fractions of the range per axis (valid: 0 <= f < 1): just below, ON the exclusive upper bound, far outside, NaN, +-inf
BAD = ([-0.06, 0.3, 0.3], [np.nan, 0.3, 0.3], [0.3, 0.3, np.inf], [0.3, 1.0, 0.3], [-np.inf, 0.3, 0.3], [0.3, 0.3, 1.0],
       [0.3, np.nan, 0.3], [0.3, 0.3, -1e-4], [1e30, 0.3, 0.3], [0.3, -1e30, 0.3])


def _bad_xyz(j, geo):
    rg = np.float32(geo["point_cloud_range"])
    with np.errstate(invalid="ignore", over="ignore"):
        return rg[:3] + np.float32(BAD[j % len(BAD)]) * (rg[3:] - rg[:3])


def _spoil(rng, pts, geo, keep=()):
    """about a tenth of the points made invalid (BAD)"""
    bad = np.flatnonzero(rng.random(len(pts)) < 0.1)
    for j, i in enumerate(bad[~np.isin(bad, keep)]):
        pts[i, :3] = _bad_xyz(j, geo)
    return pts


def beam_cloud(seed, n, c=4, geo=GRID):
    """n points whose consecutive points often share a cell (runs of 1-4, like consecutive returns of a beam); one run is forced
    across each wave boundary at 64 and each block boundary at 256 that the cloud reaches; about a tenth of the points invalid"""
    rng = np.random.default_rng(seed)
    cells = int(np.prod(grid_zyx(geo)))
    keys = np.repeat(rng.integers(0, cells, n + 1), rng.integers(1, 5, n + 1))[:n]
    keep = []
    for edge in (WAVE, BLOCK, 4 * BLOCK):
        lo, hi = edge - 2, min(edge + 2, n)
        if edge < n:
            keys[lo:hi] = keys[lo]
            keep += list(range(lo, hi))
    if n >= 2:
        keys[1] = keys[0]                                        # lane 0 starts a run
        keep += [0, 1]
    return _spoil(rng, _in_cells(rng, keys, geo, c), geo, keep)


SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)


def size_scene(n):
    return _scene(beam_cloud(100 + n, n))


def one_voxel():
    """200 points, all of them in one cell: every wave is one run, longer than P"""
    rng = np.random.default_rng(1)
    return _scene(_in_cells(rng, np.full(200, 91), GRID, 4))


def one_voxel_run():
    """200 points: 50 scattered ones, then a run of 100 in one cell from lane 50 of the first wave across the boundaries at 64 and
    128, then 50 scattered ones of which some come back to that cell"""
    rng = np.random.default_rng(2)
    keys = np.concatenate([rng.integers(0, 256, 50), np.full(100, 91), rng.integers(0, 256, 50)])
    keys[[160, 161, 190]] = 91
    return _scene(_in_cells(rng, keys, GRID, 4))


def per_voxel_cap(P):
    """1025 points over 256 cells: P = 1 below almost every count, P = 35 above every count"""
    return _scene(beam_cloud(3, 1025), P=P)


def every_cell_cap():
    """all 256 cells occupied (each first met in shuffled order among 700 points), max_voxels = 100"""
    rng = np.random.default_rng(4)
    keys = np.concatenate([rng.permutation(256), rng.integers(0, 256, 444)])
    keys = keys[rng.permutation(len(keys))]
    return _scene(_in_cells(rng, keys, GRID, 4), max_voxels=100)


def late_voxels_cap():
    """a shuffled cloud of 1025 points, max_voxels = 100: the voxels that first appear after the 100th are dropped, while points of
    the kept voxels keep arriving among them"""
    rng = np.random.default_rng(5)
    pts = beam_cloud(6, 1025)
    return _scene(pts[rng.permutation(len(pts))], max_voxels=100)


def no_points(c=4):
    return _scene(np.zeros((0, c), np.float32))


def all_outside():
    """300 points, none of them in the range: an empty occupancy bitmap"""
    rng = np.random.default_rng(7)
    pts = _in_cells(rng, rng.integers(0, 256, 300), GRID, 4)
    for i in range(300):
        pts[i, :3] = _bad_xyz(i, GRID)
    return _scene(pts)


def waymo_sparse():
    """2000 points on the Waymo grid: a few thousand bits in a bitmap of 9.05e7 cells"""
    return _scene(beam_cloud(8, 2000, c=5, geo=WAYMO), geo=WAYMO, max_voxels=150000)


def channels(c):
    return _scene(beam_cloud(9, 257, c=c))


SCENES = {"n%d" % n: (lambda n=n: size_scene(n)) for n in SIZES}
SCENES.update(one_voxel=one_voxel, one_voxel_run=one_voxel_run, P1=lambda: per_voxel_cap(1), P35=lambda: per_voxel_cap(35),
              every_cell_cap=every_cell_cap, late_voxels_cap=late_voxels_cap, no_points=no_points, all_outside=all_outside,
              waymo_sparse=waymo_sparse, c3=lambda: channels(3), c4=lambda: channels(4), c5=lambda: channels(5))
COORD_PARAMS = [(cols, b) for cols in (3, 4) for b in (0, 3)]          # (coord_cols, batch_idx) of cpd_voxelize
RAW_SCENES = ("no_points", "n257", "late_voxels_cap")                 # scenes of the raw C-ABI call with sentinels behind every output
