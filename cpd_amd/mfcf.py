"""GPU drop-in for CPD's MFCF pseudo-label generator (cpd/unsupervised_core/mfcf.py, with outline_utils.py voxel_sampling,
OutlineFitter.box_fit_DGD, density_guided_drift, correct_orientation, correct_heading and TrackSmooth): <seq>/<seq>.pkl, the
NNNN.npy frames and ppscore/NNNN.npy go in, <seq>/<seq>_outline_MFCF.pkl comes out -- the file the C_PROTO refiner
(cpd_amd.cproto, cpd_amd.cproto_refine) starts from. Per chunk of frames the aggregation over the window, voxel_sampling, ground
removal, DBSCAN, box_fit and the three box corrections run as HIP kernels (csrc/mfcf.hip, csrc/outline.hip) with one copy back;
the tracker over the per-frame boxes is cpd_amd.tracker on the host.

Exactness contract: the aggregated rows, the voxel-sampled rows and their order are the reference's bit for bit;
the boxes agree to 1e-9 except where the open hull (§5l) or the float32 inverse (§5o) picks another rectangle or bin.
Deviations, all raised: frame_num % frame_interval != 0 (the reference never meets j == i and fails on None), more than 16 sweeps
in a window, a ppscore file whose length is not its frame's, point dtypes other than float16 / float32, PP scores other than
float16.
"""
import copy
import ctypes
import os
import pickle as pkl
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import outline
from .outline import DBSCAN_GENERATOR_CONFIG, _get, _paths
from .seq_io import SweepCache, dispatch_outline_box, frame_path, gpu_modules, run_sequences
from .tracker import TrackSmooth

# GeneratorConfig of tools/cfgs/dataset_configs/waymo_unsupervised/waymo_unsupervised_cproto.yaml: the aggregation, the
# OutlineFitter arguments and the tracker block
MFCF_GENERATOR_CONFIG = dict(
    DBSCAN_GENERATOR_CONFIG, frame_num=5, frame_interval=1, ppscore_thresh=0.7,
    state_func_covariance=10, measure_func_covariance=0.1, prediction_score_decay=0.025, LiDAR_scanning_frequency=10,
    max_prediction_num=16, max_prediction_num_for_new_object=3, lwh_win_size=0, yaw_win_size=0, smoothing_method='mean',
    input_score=-0.5, init_score=-0.5, update_score=-0.5, post_score=1.4, latency=-1, remove_short_track=0)
MFCF_CONFIG = dict(InitLabelGenerator='MFCF', GeneratorConfig=MFCF_GENERATOR_CONFIG)

MAX_WINDOW = 16        # mfcf.hip MF_MAX_WINDOW
STEP_DRIFT, STEP_ORIENT, STEP_HEADING, STEP_ALL_ROWS = 1, 2, 4, 8
BIT_DRIFT_X, BIT_DRIFT_Y, BIT_ORIENT_X, BIT_ORIENT_MAX, BIT_TURNED, BIT_FLIPPED = 1, 2, 4, 8, 16, 32


def _check_points(points):
    points = np.asarray(points)
    if points.dtype not in (np.float16, np.float32):
        raise TypeError("cpd_amd.mfcf: points must be float16 or float32 (got %s)" % points.dtype)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError("cpd_amd.mfcf: points must be [N, >=3]")
    return points


def _check_scores(h, n_rows, where=""):
    h = np.asarray(h)
    if h.dtype != np.float16:
        raise TypeError("cpd_amd.mfcf: PP scores must be float16, as cpd_amd.ppscore stores them (got %s%s); the threshold "
                        "test is numpy's in that dtype" % (h.dtype, where))
    if h.ndim != 1 or len(h) != n_rows:
        raise ValueError("cpd_amd.mfcf: %d PP scores for a frame of %d rows%s" % (h.size, n_rows, where))
    return h


def window(i, frame_num, frame_interval, exists):
    """The sweeps frame i aggregates, in loop order (mfcf.py:53-57): range(i - frame_num, i + frame_num, frame_interval) over
    the frames for which exists(j); a negative j names a file that never exists."""
    if frame_interval <= 0 or frame_num <= 0:
        raise ValueError("cpd_amd.mfcf: frame_num and frame_interval must be positive")
    if frame_num % frame_interval != 0:
        raise ValueError("cpd_amd.mfcf: frame_num (%d) must be a multiple of frame_interval (%d): the window of frame i must "
                         "hold frame i itself" % (frame_num, frame_interval))
    js = [j for j in range(i - frame_num, i + frame_num, frame_interval) if j >= 0 and exists(j)]
    if len(js) > MAX_WINDOW:
        raise NotImplementedError("cpd_amd.mfcf: at most %d sweeps in a window (frame_num %d, frame_interval %d give %d)"
                                  % (MAX_WINDOW, frame_num, frame_interval, len(js)))
    return js


def threshold_f16(thresh):
    """The Python float as numpy 2 rounds it when it meets a float16 array (all_H > thresh, mfcf.py:71)."""
    return float(np.float16(thresh))


class MFCFGPU:
    """The per-frame launch sequence on one device: gather, voxel_sample, ground, dbscan, boxes, fit_dgd, one copy back."""

    def __init__(self, generator_cfg=None, device=None, ol=None):
        cfg = MFCF_GENERATOR_CONFIG if generator_cfg is None else generator_cfg
        self.ol = ol if ol is not None else outline.OutlineGPU(outline._params(cfg), device)   # ol: an OutlineGPU to share
        self.device, self.ws = self.ol.device, self.ol.ws

    # -- stages (device tensors in, device tensors out) --
    def upload(self, points, scores=None):
        """A sweep's x y z rows in their dtype (and its float16 PP scores) on the device."""
        torch, _ = gpu_modules()
        points = _check_points(points)
        pts = torch.from_numpy(np.ascontiguousarray(points[:, 0:3])).to(self.device)
        if scores is None:
            return pts, None
        h = torch.from_numpy(np.ascontiguousarray(_check_scores(scores, len(points)))).to(self.device)
        return pts, h

    def gather(self, sweeps, poses, windows, current, thresh):
        """sweeps: list of (pts, h) device pairs; poses: their 4x4 matrices; windows[f]: indices into sweeps in loop order;
        current[f]: the frame's own sweep. Returns (rows [n, 3] float32, off [F + 1] device, count [F] device, off host)."""
        torch, _lib = gpu_modules()
        lib, F, S = _lib.lib(), len(windows), len(sweeps)
        rows = np.array([int(p.shape[0]) for p, _ in sweeps], np.int32)
        if any(len(w) > MAX_WINDOW for w in windows):
            raise NotImplementedError("cpd_amd.mfcf: at most %d sweeps in a window" % MAX_WINDOW)
        win = np.full((F, MAX_WINDOW), -1, np.int32)
        for f, w in enumerate(windows):
            win[f, :len(w)] = w
        win_count = np.array([len(w) for w in windows], np.int32)
        cur = np.asarray(current, np.int32)
        off = np.zeros(F + 1, np.int32)
        off[1:] = np.cumsum([rows[list(w)].sum() + rows[c] for w, c in zip(windows, cur)])
        n = int(off[-1])
        pose = np.ascontiguousarray(np.stack([np.asarray(p, np.float64).reshape(16) for p in poses])) if S else np.zeros((1, 16))
        inv = np.ascontiguousarray(np.stack([np.linalg.inv(np.asarray(poses[c], np.float64)).reshape(16) for c in cur]))
        ptrs = np.array([p.data_ptr() for p, _ in sweeps], np.uint64)
        hptrs = np.array([h.data_ptr() if h is not None else 0 for _, h in sweeps], np.uint64)
        stride = np.array([int(p.stride(0)) if p.shape[0] else 3 for p, _ in sweeps], np.int32)
        half = np.array([1 if p.dtype == torch.float16 else 0 for p, _ in sweeps], np.int32)
        out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        count = torch.empty(F, dtype=torch.int32, device=self.device)
        nb = lib.cpd_mfcf_gather_workspace_bytes(int(np.diff(off).max()) if F else 0)
        ws = self.ws.get("mfcf_gather", nb)
        vp, ip, dp = lambda a: ctypes.c_void_p(a.ctypes.data), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        _lib.check(lib.cpd_mfcf_gather(vp(ptrs), vp(hptrs), rows.ctypes.data_as(ip), stride.ctypes.data_as(ip),
                                       half.ctypes.data_as(ip), pose.ctypes.data_as(dp), S, win.ctypes.data_as(ip),
                                       win_count.ctypes.data_as(ip), cur.ctypes.data_as(ip), inv.ctypes.data_as(dp),
                                       off.ctypes.data_as(ip), F, threshold_f16(thresh), _lib.ptr(out), _lib.ptr(count),
                                       _lib.ptr(ws), nb, _lib.stream()), "cpd_mfcf_gather")
        return out, torch.from_numpy(off).to(self.device), count, off

    def voxel_sample(self, rows, off, count, n_frames, res=0.1):
        """Returns (out [n, 3], out_src [n], out_off [F + 2], err [1])."""
        torch, _lib = gpu_modules()
        lib, n = _lib.lib(), int(rows.shape[0])
        out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        src = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        out_off = torch.empty(n_frames + 2, dtype=torch.int32, device=self.device)
        err = torch.zeros(1, dtype=torch.int32, device=self.device)
        nb = lib.cpd_mfcf_voxel_sample_workspace_bytes(n_frames, n)
        ws = self.ws.get("mfcf_voxel", nb)
        _lib.check(lib.cpd_mfcf_voxel_sample(_lib.ptr(rows), _lib.ptr(off), _lib.ptr(count), n_frames, n, float(np.float32(res)),
                                             _lib.ptr(out), _lib.ptr(src), _lib.ptr(out_off), _lib.ptr(err), _lib.ptr(ws), nb,
                                             _lib.stream()), "cpd_mfcf_voxel_sample")
        return out, src, out_off, err

    def fit_dgd(self, xyz, off, cnt, labels, boxes, n_frames, cap, steps=STEP_DRIFT | STEP_ORIENT | STEP_HEADING):
        """boxes: cpd_outline_boxes' output for the same frames and cap. Returns (out [cap, 7], bits [cap], n_out [1])."""
        torch, _lib = gpu_modules()
        out = torch.empty((max(cap, 1), 7), dtype=torch.float64, device=self.device)
        bits = torch.zeros(max(cap, 1), dtype=torch.int32, device=self.device)
        n_out = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().cpd_mfcf_fit_dgd(_lib.ptr(xyz), _lib.ptr(off), _lib.ptr(cnt), n_frames, int(xyz.shape[0]),
                                               _lib.ptr(labels), _lib.ptr(boxes), int(cap), int(steps), _lib.ptr(out),
                                               _lib.ptr(bits), _lib.ptr(n_out), _lib.stream()), "cpd_mfcf_fit_dgd")
        return out, bits, n_out

    # -- the chain from aggregated rows on: every launch, then one copy back --
    def sampled_boxes(self, rows, off, count, n_frames, stages=False):
        """rows / off / count: gather's output (or any float32 slices). Per frame the box_fit_DGD boxes ([K, 7] float64, or []
        as the reference returns it); with stages also the branch bits per frame and the voxel-sampled rows per frame."""
        torch, _lib = gpu_modules()
        from .cproto import _copy_back
        vox, _, vox_off, verr = self.voxel_sample(rows, off, count, n_frames)
        F1 = n_frames + 1                                    # the zeroed tail is one more frame without non-ground rows
        xyz, _, cnt, gerr = self.ol.ground(vox, vox_off, F1)
        labels, ncl = self.ol.dbscan(xyz, vox_off, cnt, F1)
        cap = outline.BOX_CAP_PER_FRAME * n_frames
        while True:
            bx = self.ol.boxes(xyz, vox_off, cnt, labels, ncl, F1, True, cap)
            out, bits, _ = self.fit_dgd(xyz, vox_off, cnt, labels, bx, F1, cap)
            back = [("counts", bx[:F1]), ("box", out), ("bits", bits), ("gerr", gerr), ("verr", verr)]
            if stages:
                back += [("vox_off", vox_off), ("vox", vox)]
            res = _copy_back(back)
            if int(res["verr"][0]):
                raise _lib.CpdHipError("cpd_mfcf_voxel_sample failed: CPD_ERR_UNSUPPORTED (a NaN coordinate, or a cloud "
                                       "wider than 2^21 cells)")
            if int(res["gerr"][0]):
                raise _lib.CpdHipError("cpd_outline_ground: segment index outside the table")
            counts = res["counts"].astype(np.int64)
            if counts.sum() <= cap:
                break
            cap = int(counts.sum())      # rare: more boxes than the default capacity; the box stages again with room for all
        boxes, all_bits, o = [], [], 0
        for c in counts[:n_frames]:
            b = res["box"][o:o + c].copy()
            boxes.append(b if len(b) else [])
            all_bits.append(res["bits"][o:o + c].copy())
            o += c
        if not stages:
            return boxes
        vo = res["vox_off"]
        return boxes, all_bits, [res["vox"][vo[f]:vo[f + 1]].copy() for f in range(n_frames)]

    def frames_boxes(self, sweeps, poses, windows, current, thresh, stages=False):
        rows, off, count, _ = self.gather(sweeps, poses, windows, current, thresh)
        return self.sampled_boxes(rows, off, count, len(windows), stages)


_GPU = {}


def _gpu(device=None, cfg=None):
    torch, _ = gpu_modules()
    dev = torch.device(device if device is not None else "cuda")
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    g = _GPU.get(key)
    if g is None:
        g = _GPU[key] = MFCFGPU(cfg, dev)
    return g


# ---- one call on the GPU each (reference signatures) ----------------------------------------------------------------------------

def voxel_sampling(point2, res_x=0.1, res_y=0.1, res_z=0.1, device=None):
    """outline_utils.py:368-389 for float32 rows [N, >=3]: one row per 0.1 m cell, cells in the order of their first row, each
    with its last row (all columns). float32 only: the cell arithmetic runs in the rows' dtype."""
    torch, _ = gpu_modules()
    point2 = np.asarray(point2)
    if point2.dtype != np.float32:
        raise TypeError("cpd_amd.mfcf: voxel_sampling takes float32 rows (got %s): the cell quotient is computed in the "
                        "rows' dtype" % point2.dtype)
    if not (res_x == res_y == res_z):
        raise NotImplementedError("cpd_amd.mfcf: one cell size for the three axes")
    n = len(point2)
    if n == 0:
        raise ValueError("cpd_amd.mfcf: voxel_sampling of an empty cloud (the reference fails on its minimum)")
    g = _gpu(device)
    rows = torch.from_numpy(np.ascontiguousarray(point2[:, 0:3])).to(g.device)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=g.device)
    _, src, out_off, err = g.voxel_sample(rows, i32([0, n]), i32([n]), 1, res_x)
    if int(err.item()):
        _, _lib = gpu_modules()
        raise _lib.CpdHipError("cpd_mfcf_voxel_sample failed: CPD_ERR_UNSUPPORTED (a NaN coordinate, or a cloud wider than "
                               "2^21 cells)")
    m = int(out_off[1].item())
    return point2[src[:m].cpu().numpy().astype(np.int64)]


def _dgd_one(g, points_list, boxes, steps):
    """The corrections on given boxes [K, 7], box k with the rows of points_list[k]."""
    torch, _ = gpu_modules()
    xyz = np.concatenate([outline._exact_f32(np.asarray(p)[:, 0:3]) for p in points_list], 0)
    lab = np.concatenate([np.full(len(p), i, np.int32) for i, p in enumerate(points_list)])
    n, k = len(xyz), len(points_list)
    table = np.zeros(1 + 8 * k, np.float64)
    table[0] = k
    table[1:].reshape(k, 8)[:, :7] = np.asarray(boxes, np.float64).reshape(k, 7)
    table[1:].reshape(k, 8)[:, 7] = np.arange(k)
    dev = g.device
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    out, bits, _ = g.fit_dgd(torch.from_numpy(xyz).to(dev), i32([0, n]), i32([n]), torch.from_numpy(lab).to(dev),
                             torch.from_numpy(table).to(dev), 1, k, steps)
    return out[:k].cpu().numpy(), bits[:k].cpu().numpy()


def correct_heading(orin_points, box, parts=10, device=None):
    """outline_utils.py:444-485 for one cluster [N, >=3] and one box [1, 7]: the box itself, or a copy turned by pi."""
    if parts != 10:
        raise NotImplementedError("cpd_amd.mfcf: correct_heading's ten slabs are fixed in the kernel")
    if len(orin_points) == 0:
        raise ValueError("cpd_amd.mfcf: an empty cluster has no heading")
    out, bits = _dgd_one(_gpu(device), [orin_points], np.asarray(box, np.float64).reshape(1, 7), STEP_HEADING | STEP_ALL_ROWS)
    if not bits[0] & BIT_FLIPPED:
        return box
    new_box = copy.deepcopy(box)
    new_box[0, 6] = out[0, 6]
    return new_box


class OutlineFitter(outline.OutlineFitter):
    """outline.OutlineFitter with box_fit_DGD (outline_utils.py:848-889)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.mfcf = MFCFGPU(ol=self.gpu)

    def box_fit_DGD(self, points_list, offset=0.2, return_bits=False):
        if offset != 0.2:
            raise NotImplementedError("cpd_amd.mfcf: box_fit_DGD's offset is fixed at 0.2 in the kernel")
        torch, _ = gpu_modules()
        points_list = [p for p in points_list if len(p)]     # an empty cluster raises in the reference: skipped
        if not points_list:
            return ([], np.zeros(0, np.int32)) if return_bits else []
        g, dev = self.gpu, self.gpu.device
        xyz = np.concatenate([outline._exact_f32(np.asarray(p)[:, 0:3]) for p in points_list], 0)
        lab = np.concatenate([np.full(len(p), i, np.int32) for i, p in enumerate(points_list)])
        n, k = len(xyz), len(points_list)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        t_xyz, off, cnt, t_lab = torch.from_numpy(xyz).to(dev), i32([0, n]), i32([n]), torch.from_numpy(lab).to(dev)
        bx = g.boxes(t_xyz, off, cnt, t_lab, i32([k]), 1, False, k)
        out, bits, n_out = self.mfcf.fit_dgd(t_xyz, off, cnt, t_lab, bx, 1, k)
        m = int(n_out.item())
        boxes = out[:m].cpu().numpy() if m else []
        return (boxes, bits[:m].cpu().numpy()) if return_bits else boxes


# ---- the generator ---------------------------------------------------------------------------------------------------------------

def _load_pair(seq_dir, j):
    path = frame_path(seq_dir, j)
    if not os.path.exists(path):
        return None
    pts = np.load(path)[:, 0:3]
    h_path = frame_path(os.path.join(seq_dir, 'ppscore'), j)
    if not os.path.exists(h_path):
        raise FileNotFoundError("cpd_amd.mfcf: %s is missing (run cpd_amd.ppscore.create_ppscore first)" % h_path)
    return pts, np.load(h_path)


class MFCF:
    """mfcf.py MFCF: the same file contract (<seq>/<seq>.pkl, NNNN.npy, ppscore/NNNN.npy in, <seq>/<seq>_outline_MFCF.pkl out,
    cached: an existing output is returned as it is)."""

    def __init__(self, seq_name, root_path, config, device=None, chunk=16):
        self.seq_name, self.root_path, self.dataset_cfg = seq_name, root_path, config
        self.device, self.chunk = device, int(chunk)
        self._gpu = None
        if self.chunk < 1:
            raise ValueError("cpd_amd.mfcf: chunk must be at least 1")

    @property
    def gpu(self):
        if self._gpu is None:
            self._gpu = MFCFGPU(_get(self.dataset_cfg, "GeneratorConfig"), self.device)
        return self._gpu

    def per_frame_boxes(self, infos, pool=None, stages=False):
        """mfcf.py:46-80: the per-frame boxes of every frame of infos (and the poses). A sweep is read once (on the pool, a
        chunk ahead of its first use), uploaded once and dropped after its last window."""
        gcfg = _get(self.dataset_cfg, "GeneratorConfig")
        frame_num, inte = int(_get(gcfg, "frame_num")), int(_get(gcfg, "frame_interval"))
        thresh = _get(gcfg, "ppscore_thresh")
        seq_dir = os.path.join(self.root_path, self.seq_name)
        n = len(infos)
        window(0, frame_num, inte, lambda j: False)          # the argument checks, before any file is read
        window(frame_num, frame_num, inte, lambda j: j < n)
        own_pool = pool is None
        pool = ThreadPoolExecutor(4) if own_pool else pool

        def upload(j, pair):
            _check_scores(pair[1], len(pair[0]), " (%s frame %d)" % (self.seq_name, j))
            return self.gpu.upload(*pair)

        cache = SweepCache(pool, n, lambda j: _load_pair(seq_dir, j), upload)

        def span(c0):      # the frames the chunk that starts at c0 touches
            return range(max(0, c0 - frame_num), min(n, min(n, c0 + self.chunk) - 1 + frame_num))

        all_labels, all_bits, all_vox = [], [], []
        try:
            for j in span(0):
                cache.want(j)
            for c0 in range(0, n, self.chunk):
                c1 = min(n, c0 + self.chunk)
                cache.drop_before(c0 - frame_num)
                # negative j never exists as a file; j >= len(infos) would fail on infos[j] in the reference, here it is skipped
                wins = [window(i, frame_num, inte, lambda j: j < n and cache.get(j) is not None) for i in range(c0, c1)]
                for i, w in zip(range(c0, c1), wins):
                    if i not in w:
                        raise FileNotFoundError("cpd_amd.mfcf: %s is missing: frame %d is not in its own window"
                                                % (frame_path(seq_dir, i), i))
                for j in span(c1):                           # the next chunk's reads overlap this chunk's kernels
                    cache.want(j)
                used = sorted(set(j for w in wins for j in w))
                index = {j: k for k, j in enumerate(used)}
                res = self.gpu.frames_boxes([cache.get(j) for j in used], [infos[j]['pose'] for j in used],
                                            [[index[j] for j in w] for w in wins], [index[i] for i in range(c0, c1)], thresh,
                                            stages)
                if stages:
                    all_labels += res[0]
                    all_bits += res[1]
                    all_vox += res[2]
                else:
                    all_labels += res
        finally:
            if own_pool:
                pool.shutdown()
        all_pose = [info['pose'] for info in infos]
        return (all_labels, all_pose, all_bits, all_vox) if stages else (all_labels, all_pose)

    def generate_outline_box(self, pool=None):
        method = _get(self.dataset_cfg, "InitLabelGenerator")
        in_pkl, out_pkl = _paths(self.seq_name, self.root_path, method)
        if os.path.exists(out_pkl):
            with open(out_pkl, 'rb') as f:
                return pkl.load(f)
        with open(in_pkl, 'rb') as f:
            infos = pkl.load(f)
        all_labels, all_pose = self.per_frame_boxes(infos, pool)
        tracker = TrackSmooth(_get(self.dataset_cfg, "GeneratorConfig"))
        tracker.tracking(all_labels, all_pose)
        for i in range(len(infos)):
            objs, ids, cls, dif = tracker.get_current_frame_objects_and_cls(i)
            infos[i]['outline_box'], infos[i]['outline_ids'] = objs, ids
            infos[i]['outline_cls'], infos[i]['outline_dif'] = cls, dif
        with open(out_pkl, 'wb') as f:
            pkl.dump(infos, f)
        return infos

    def __call__(self):
        return self.generate_outline_box()


def create_mfcf(seq_names, root_path, dataset_cfg, device=None, chunk=16):
    """Single-process sequence driver in place of the dataset's multiprocessing.Pool(16) (forked workers must not each open the
    GPU): every sequence through one GPU context, the .npy and ppscore reads on a small thread pool while the GPU works."""
    with ThreadPoolExecutor(4) as pool:
        return run_sequences(lambda s: MFCF(s, root_path, dataset_cfg, device, chunk), seq_names,
                             lambda m: m.generate_outline_box(pool))


def compute_outline_box(seq_name, root_path, dataset_cfg):
    """cpd/unsupervised_core/__init__.py compute_outline_box for what has a GPU drop-in: InitLabelGenerator 'DBSCAN'
    (outline.DBSCAN) and 'MFCF', LabelRefiner 'C_PROTO' (cproto_refine.C_PROTO). outline.compute_outline_box keeps its own,
    narrower contract."""
    return dispatch_outline_box(seq_name, root_path, dataset_cfg, {'DBSCAN': outline.DBSCAN, 'MFCF': MFCF}, ('C_PROTO',), "mfcf")
