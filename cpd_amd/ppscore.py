"""GPU drop-in for CPD's PP-score precompute (cpd/unsupervised_core/precompute_ppscore.py): for every point of a frame the
number of points within max_neighbor_dist in each neighbouring traversal, and the normalised entropy H of those counts that
MFCF thresholds (ppscore_thresh). One call of cpd_ppscore (csrc/ppscore.hip) serves one current frame: both rigid transforms,
a hashed grid over all traversals, the counts and H.

Exactness contract: the transformed coordinates and the counts are the reference's bit for bit; H is the
reference's float16 except where its float64 value lies within 1e-9 of a float16 rounding tie (the device log may differ
from numpy's in the last bits), there within one float16 step. Deviations: fewer than two traversals give H = NaN for every
point and a warning (the reference divides by log(1) = 0 and stores +-inf / NaN); a window that does not hold the current
frame's own file raises FileNotFoundError (the reference fails on None).
"""
import ctypes
import os
import pickle as pkl
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .seq_io import SweepCache, frame_path

MAX_TRAVERSALS = 16    # ppscore.hip PP_MAX_TRAV


def _check_points(points):
    points = np.asarray(points)
    if points.dtype not in (np.float16, np.float32):
        raise TypeError("cpd_amd.ppscore: points must be float16 or float32 (got %s)" % points.dtype)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError("cpd_amd.ppscore: points must be [N, >=3]")
    return points


def _mat16(m):
    m = np.ascontiguousarray(np.asarray(m, np.float64))
    if m.shape != (4, 4):
        raise ValueError("cpd_amd.ppscore: a pose is a 4x4 matrix")
    return m


class PPScoreGPU:
    """cpd_ppscore on one device: workspace and outputs grow to the largest frame seen and are reused."""

    def __init__(self, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        self.ws = None
        self.counts = None
        self.h = None

    def upload(self, points):
        """[N, >=3] float16 / float32 host rows -> device rows (all columns: the kernel reads with the row stride)."""
        return torch.from_numpy(np.ascontiguousarray(_check_points(points))).to(self.device)

    def _grow(self, name, numel, dtype):
        b = getattr(self, name)
        if b is None or b.numel() < numel:
            b = torch.empty(max(int(numel), 64), dtype=dtype, device=self.device)
            setattr(self, name, b)
        return b

    def run(self, query, travs, poses=None, cur_pose_inv=None, radius=0.3, want_counts=True, want_h=True):
        """query: device [N, C]; travs: list of device [M_t, C_t] tensors of float16 / float32. Returns device views (counts
        [N, T] int32 or None, h [N] float16 or None) into buffers the next call overwrites."""
        lib = _lib.lib()
        n_trav = len(travs)
        if n_trav > MAX_TRAVERSALS:
            raise _lib.CpdHipError("cpd_ppscore failed: CPD_ERR_UNSUPPORTED (%d traversals, at most %d)" % (n_trav, MAX_TRAVERSALS))
        for t in [query] + list(travs):
            if t.dtype not in (torch.float16, torch.float32):
                raise TypeError("cpd_amd.ppscore: points must be float16 or float32 (got %s)" % t.dtype)
        n = int(query.shape[0])
        off = np.zeros(n_trav + 1, np.int32)
        off[1:] = np.cumsum([int(t.shape[0]) for t in travs])
        if n_trav == 0:
            ref = torch.zeros((1, 3), dtype=torch.float32, device=self.device)
        elif n_trav == 1:
            ref = travs[0]
        else:   # one dtype and one row width per call: the first three columns, widened exactly where the dtypes differ
            dt = torch.float16 if all(t.dtype == torch.float16 for t in travs) else torch.float32
            ref = torch.cat([t[:, :3].to(dt) for t in travs], 0)
        if ref.shape[0] and ref.stride(1) != 1:
            ref = ref.contiguous()
        if n and query.stride(1) != 1:
            query = query.contiguous()
        nb = lib.cpd_ppscore_workspace_bytes(n, int(off[-1]), n_trav)
        ws = self._grow("ws", nb, torch.uint8)
        counts = self._grow("counts", n * max(n_trav, 1), torch.int32) if want_counts else None
        h = self._grow("h", n, torch.float16) if want_h else None
        dp = ctypes.POINTER(ctypes.c_double)
        p_poses = p_inv = None
        if poses is not None:
            pm = np.ascontiguousarray(np.stack([_mat16(p) for p in poses]).reshape(n_trav, 16)) if n_trav else np.zeros((1, 16))
            im = _mat16(cur_pose_inv)
            p_poses, p_inv = pm.ctypes.data_as(dp), im.ctypes.data_as(dp)
        _lib.check(lib.cpd_ppscore(ctypes.c_void_p(query.data_ptr()), n, int(query.stride(0)) if n else 3,
                                   1 if query.dtype == torch.float16 else 0, ctypes.c_void_p(ref.data_ptr()),
                                   off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n_trav,
                                   int(ref.stride(0)) if ref.shape[0] else 3, 1 if ref.dtype == torch.float16 else 0,
                                   p_poses, p_inv, float(radius), _lib.ptr(counts), _lib.ptr(h), _lib.ptr(ws), nb,
                                   _lib.stream()), "cpd_ppscore")
        return (counts[:n * n_trav].view(n, n_trav) if want_counts else None), (h[:n] if want_h else None)


_GPU = {}


def _gpu(device=None):
    dev = torch.device(device if device is not None else "cuda")
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    g = _GPU.get(key)
    if g is None:
        g = _GPU[key] = PPScoreGPU(dev)
    return g


def _as_list(traversals):
    return list(traversals.values()) if isinstance(traversals, dict) else list(traversals)


def count_neighbors(ptc, traversals, max_neighbor_dist=0.3, device=None):
    """count_neighbors (l.8-14) with the traversals' point arrays (a list, or a dict in its order) in place of the dict of
    cKDTrees: [N, T] int64, the points of each traversal within max_neighbor_dist (inclusive) of every row of ptc."""
    g = _gpu(device)
    travs = [g.upload(t) for t in _as_list(traversals)]
    counts, _ = g.run(g.upload(ptc), travs, radius=max_neighbor_dist, want_h=False)
    return counts.cpu().numpy().astype(np.int64)


def compute_ephe_score(count):
    """compute_ephe_score (l.16-21), the reference's numpy expression (host; the GPU path computes H in cpd_ppscore)."""
    count = np.asarray(count)
    N = count.shape[1]
    P = count / (np.expand_dims(count.sum(axis=1), -1) + 1e-8)
    H = (-P * np.log(P + 1e-8)).sum(axis=1) / np.log(N)
    return H


def compute_ppscore(cur_frame, neighbor_traversals=None, max_neighbor_dist=0.3, device=None):
    """compute_ppscore (l.23-34): H [N] float64 of cur_frame against traversals that are already in its coordinates."""
    return compute_ephe_score(count_neighbors(cur_frame, neighbor_traversals, max_neighbor_dist, device))


def points_rigid_transform(cloud, pose):
    """points_rigid_transform (l.36-45) on the host: [N, >=3] -> [N, 3] float32 through the float64 matrix product (the
    drivers below never call it: cpd_ppscore applies both transforms on the device)."""
    if cloud.shape[0] == 0:
        return cloud
    mat = np.ones(shape=(cloud.shape[0], 4), dtype=np.float32)
    mat[:, 0:3] = cloud[:, 0:3]
    return np.array((np.asarray(pose) @ mat.astype(np.float64).T).T, dtype=np.float32)[:, 0:3]


def _load(path):
    return np.load(path) if os.path.exists(path) else None


def _sequence(gpu, pool, seq_name, root_path, max_win, win_inte, max_neighbor_dist):
    seq_dir = os.path.join(root_path, seq_name)
    out_dir = os.path.join(seq_dir, 'ppscore')
    with open(os.path.join(seq_dir, seq_name + '.pkl'), 'rb') as f:
        infos = pkl.load(f)
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    n = len(infos)
    cache = SweepCache(pool, n, lambda j: _load(frame_path(seq_dir, j)), lambda j, host: gpu.upload(host))
    ahead = max_win + 4
    for j in range(min(n, ahead)):
        cache.want(j)
    warned = False
    for i in range(n):
        cache.want(i + ahead - 1)
        cache.drop_before(i - max_win)
        # negative j never exists as a file; j >= len(infos) would fail on infos[j] in the reference, here it is skipped
        js = [j for j in range(i - max_win, i + max_win, win_inte) if 0 <= j < n and cache.get(j) is not None]
        if i not in js:
            raise FileNotFoundError("cpd_amd.ppscore: frame %s is not in its own window (max_win %d, win_inte %d) or its "
                                    "file is missing" % (frame_path(seq_dir, i), max_win, win_inte))
        if len(js) < 2 and not warned:
            warnings.warn("cpd_amd.ppscore: %s has frames with fewer than two traversals; their PP score is NaN" % seq_name)
            warned = True
        _, h = gpu.run(cache.get(i), [cache.get(j) for j in js], [infos[j]['pose'] for j in js],
                       np.linalg.inv(infos[i]['pose']), max_neighbor_dist, want_counts=False)
        np.save(frame_path(out_dir, i), h.cpu().numpy())
    return True


def save_pp_score(seq_name, root_path, max_win=30, win_inte=5, max_neighbor_dist=0.3, device=None):
    """save_pp_score (l.48-102): <root>/<seq>/ppscore/NNNN.npy (float16 [N]) for every frame of <root>/<seq>/<seq>.pkl, always
    recomputed; the window is the reference's range(i - max_win, i + max_win, win_inte) over the frame files that exist."""
    with ThreadPoolExecutor(4) as pool:
        return _sequence(_gpu(device), pool, seq_name, root_path, max_win, win_inte, max_neighbor_dist)


def create_ppscore(seq_names, root_path, max_win=30, win_inte=5, max_neighbor_dist=0.3, device=None):
    """Single-process sequence driver in place of Dataset.create_ppscore's multiprocessing.Pool(16) (forked workers must not
    each open the GPU): every sequence through one GPU context, .npy reads on a small thread pool while the GPU works."""
    gpu = _gpu(device)
    with ThreadPoolExecutor(4) as pool:
        return [_sequence(gpu, pool, s, root_path, max_win, win_inte, max_neighbor_dist) for s in seq_names]
