"""GPU drop-in for CPD's DBSCAN pseudo-label generator (cpd/unsupervised_core/dbscan.py, outline_utils.py OutlineFitter,
ground_removal.py Processor): ground removal, DBSCAN clustering and box fitting run as HIP kernels (csrc/outline.hip) on a
batch of frames per launch; the class chain (get_box_cls) and drop_cls stay vectorised numpy on the host.

Exactness contract: the non-ground points and their order, the DBSCAN labels and the classes are the
reference's; boxes agree to 1e-9 except where the reference's open hull (its closing edge is omitted) picks another
rectangle -- here every hull edge is a candidate.
"""
import ctypes
import os
import pickle as pkl

import numpy as np
import torch

from . import _lib
from .seq_io import _get, _has, dispatch_outline_box, dtype_runs, frame_path, prefetched_chunks

# GeneratorConfig of tools/cfgs/dataset_configs/waymo_unsupervised/waymo_unsupervised_dbscan.yaml
DBSCAN_GENERATOR_CONFIG = dict(
    sensor_height=0, ground_min_threshold=[0.2, -0.5, -0.5], ground_min_distance=[0, 20, 40, 100], ground_max_threshold=1,
    cluster_dis=0.5, cluster_min_points=5, discard_max_height=4, min_box_volume=0.1, min_box_height=0.3,
    max_box_volume=200, max_box_len=10,
    cls={'Dis_Small': 0, 'Vehicle': 1, 'Pedestrian': 2, 'Cyclist': 3, 'Dis_Large': 4},
    cls_L={'Dis_Small': [0, 12], 'Vehicle': [0.5, 8], 'Pedestrian': [0.2, 1.], 'Cyclist': [1.3, 2.5], 'Dis_Large': [0, 12]},
    cls_W={'Dis_Small': [0, 12], 'Vehicle': [0.5, 3], 'Pedestrian': [0.2, 1.], 'Cyclist': [0.5, 1.], 'Dis_Large': [0, 12]},
    cls_H={'Dis_Small': [0, 0.8], 'Vehicle': [1., 3], 'Pedestrian': [0.8, 2.3], 'Cyclist': [1.4, 2.], 'Dis_Large': [3, 12]},
    max_top_z=3, max_width=3, max_len=12)

MAX_BANDS = 6          # len(ground_min_threshold) the kernels take (outline.hip OL_MAX_BANDS)
BOX_CAP_PER_FRAME = 256


_CLASS_CHAIN = ['Dis_Small', 'Pedestrian', 'Cyclist', 'Vehicle', 'Dis_Large']   # the range tests, in the reference's order


def get_box_cls(boxes, config):
    """OutlineFitter.get_box_cls (outline_utils.py:891-958), return_name=True: the first-match chain as np.select."""
    if len(boxes) == 0:
        return np.array(boxes), np.array([]), np.array([])
    boxes = np.asarray(boxes)
    l, w, h = boxes[:, 3], boxes[:, 4], boxes[:, 5]
    top_z = boxes[:, 2] + h / 2
    L, W, H = _get(config, "cls_L"), _get(config, "cls_W"), _get(config, "cls_H")
    conds = [(top_z > _get(config, "max_top_z")) | (w > _get(config, "max_width")) | (l > _get(config, "max_len"))]
    names = ['Dis_Large']
    for c in _CLASS_CHAIN:
        conds.append((L[c][0] < l) & (l <= L[c][1]) & (H[c][0] < h) & (h <= H[c][1]) & (W[c][0] < w) & (w <= W[c][1]))
        names.append(c)
    # np.array(list of str): the dtype is as wide as the longest name that occurs
    idx = np.select(conds, np.arange(len(names)), default=len(names))
    names.append('Dis_Small')
    cls = np.array([names[i] for i in idx])
    return boxes, cls, np.ones(len(boxes), dtype=np.int64)


def drop_cls(boxes, name, ids=None, dif=None, confi=None, proto_id=None, droped_cls=('Dis_Small', 'Dis_Large')):
    """outline_utils.py:487-504."""
    for cls_name in droped_cls:
        mask = name != cls_name
        boxes = boxes[mask]
        if ids is not None:
            ids = ids[mask]
        if dif is not None:
            dif = dif[mask]
        if confi is not None:
            confi = confi[mask]
        if proto_id is not None:
            proto_id = proto_id[mask]
        name = name[mask]
    return boxes, name, ids, dif, confi, proto_id


def _dtype_consts(dtype, ground_max_threshold):
    """Processor's Python-float constants as numpy 2 (NEP 50) rounds them against an array of `dtype`."""
    t = np.dtype(dtype).type
    c = [t(np.pi), t(2 * np.pi / 150), t(0.3), t((150 - 0.3) / 150), t(ground_max_threshold)]
    return (ctypes.c_float * 5)(*[float(v) for v in c])


def _check_points(points):
    points = np.asarray(points)
    if points.dtype not in (np.float16, np.float32):
        raise TypeError("cpd_amd.outline: points must be float16 or float32 (got %s); the ground projection's "
                        "arithmetic depends on the dtype" % points.dtype)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError("cpd_amd.outline: points must be [N, >=3]")
    return points


def _exact_f32(xyz):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    f = xyz.astype(np.float32)
    if not np.array_equal(f.astype(np.float64), xyz):
        raise ValueError("cpd_amd.outline: coordinates must be float32 values (the output of remove_ground)")
    return f


class _Workspace:
    """One growing device buffer per stage (no allocation inside a launch function)."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}

    def get(self, name, nbytes):
        b = self.bufs.get(name)
        if b is None or b.numel() < nbytes:
            b = self.bufs[name] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        return b


class OutlineGPU:
    """The three launch sequences on one device; frames go in as a list of [N_i, >=3] float16 / float32 arrays."""

    def __init__(self, params, device=None):
        self.p = params
        self.device = torch.device(device if device is not None else "cuda")
        self.ws = _Workspace(self.device)
        thr, dist = list(params["ground_min_threshold"]), list(params["ground_min_distance"])
        k = len(thr)
        if not 1 <= k <= MAX_BANDS:
            raise NotImplementedError("cpd_amd.outline: 1..%d distance bands (len(ground_min_threshold) = %d)" % (MAX_BANDS, k))
        need = max(2, k)
        if len(dist) < need:
            raise ValueError("ground_min_distance needs %d entries for %d bands" % (need, k))
        if any(dist[i + 1] < dist[i] for i in range(1, k - 1)):
            raise NotImplementedError("cpd_amd.outline: ground_min_distance must not decrease (overlapping bands)")
        self.thr = (ctypes.c_double * MAX_BANDS)(*[float(v) for v in thr] + [0.0] * (MAX_BANDS - k))
        dd = [float(v) for v in dist[:MAX_BANDS + 1]]
        self.dist = (ctypes.c_double * (MAX_BANDS + 1))(*dd + [0.0] * (MAX_BANDS + 1 - len(dd)))
        self.n_bands = k
        self.box_params = (ctypes.c_double * 8)(float(params["cluster_min_points"]), float(params["discard_max_height"]),
                                                float(params["min_box_volume"]), float(params["min_box_height"]),
                                                float(params["max_box_volume"]), float(params["max_box_len"]),
                                                float(thr[0]), float(dist[1]))

    # -- stages (device tensors in, device tensors out) --
    def ground(self, pts, off, n_frames):
        lib = _lib.lib()
        n = int(pts.shape[0])
        is_half = 1 if pts.dtype == torch.float16 else 0
        consts = _dtype_consts(np.float16 if is_half else np.float32, self.p.get("ground_max_threshold", 1))
        xyz = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        src = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        cnt = torch.empty(n_frames, dtype=torch.int32, device=self.device)
        err = torch.zeros(1, dtype=torch.int32, device=self.device)
        nb = lib.cpd_outline_ground_workspace_bytes(n_frames, n)
        ws = self.ws.get("ground", nb)
        _lib.check(lib.cpd_outline_ground(_lib.ptr(pts), is_half, int(pts.stride(0)), _lib.ptr(off), n_frames, n, consts,
                                          float(self.p["sensor_height"]), self.thr, self.dist, self.n_bands, _lib.ptr(xyz),
                                          _lib.ptr(src), _lib.ptr(cnt), _lib.ptr(err), _lib.ptr(ws), nb, _lib.stream()),
                   "cpd_outline_ground")
        return xyz, src, cnt, err

    def dbscan(self, xyz, off, cnt, n_frames):
        lib = _lib.lib()
        n = int(xyz.shape[0])
        labels = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        ncl = torch.empty(n_frames, dtype=torch.int32, device=self.device)
        nb = lib.cpd_outline_dbscan_workspace_bytes(n_frames, n)
        ws = self.ws.get("dbscan", nb)
        _lib.check(lib.cpd_outline_dbscan(_lib.ptr(xyz), _lib.ptr(off), _lib.ptr(cnt), n_frames, n,
                                          float(self.p["cluster_dis"]), 10, _lib.ptr(labels), _lib.ptr(ncl), _lib.ptr(ws), nb,
                                          _lib.stream()), "cpd_outline_dbscan")
        return labels, ncl

    def boxes(self, xyz, off, cnt, labels, ncl, n_frames, apply_filter, cap):
        lib = _lib.lib()
        n = int(xyz.shape[0])
        out = torch.empty(n_frames + 8 * cap, dtype=torch.float64, device=self.device)
        nb = lib.cpd_outline_boxes_workspace_bytes(n_frames, n)
        ws = self.ws.get("boxes", nb)
        _lib.check(lib.cpd_outline_boxes(_lib.ptr(xyz), _lib.ptr(off), _lib.ptr(cnt), n_frames, n, _lib.ptr(labels),
                                         _lib.ptr(ncl), int(apply_filter), self.box_params, int(cap), _lib.ptr(out),
                                         _lib.ptr(ws), nb, _lib.stream()), "cpd_outline_boxes")
        return out

    # -- host helpers --
    def upload(self, frames):
        frames = [_check_points(f) for f in frames]
        dt = frames[0].dtype
        if any(f.dtype != dt for f in frames):
            raise TypeError("cpd_amd.outline: one dtype per batch")
        cols = frames[0].shape[1]
        if any(f.shape[1] != cols for f in frames):
            frames, cols = [f[:, :3] for f in frames], 3
        host = np.concatenate(frames, 0) if frames else np.zeros((0, cols), dt)
        off = np.zeros(len(frames) + 1, np.int32)
        off[1:] = np.cumsum([len(f) for f in frames])
        pts = torch.from_numpy(np.ascontiguousarray(host)).to(self.device, non_blocking=False)
        return pts, torch.from_numpy(off).to(self.device), off

    def frames_boxes(self, frames):
        """Per frame the box_fit output ([K, 7] float64, or [] as the reference returns it), one read-back per call."""
        n_frames = len(frames)
        pts, off, _ = self.upload(frames)
        xyz, _, cnt, err = self.ground(pts, off, n_frames)
        labels, ncl = self.dbscan(xyz, off, cnt, n_frames)
        cap = BOX_CAP_PER_FRAME * n_frames
        out = self.boxes(xyz, off, cnt, labels, ncl, n_frames, True, cap)
        host = torch.cat([out, err.to(torch.float64)]).cpu().numpy()
        if host[-1] != 0:
            raise _lib.CpdHipError("cpd_outline_ground: segment index outside the table")
        counts = host[:n_frames].astype(np.int64)
        if counts.sum() > cap:   # rare: more boxes than the default capacity; run the box stage again with room for all
            cap = int(counts.sum())
            host = self.boxes(xyz, off, cnt, labels, ncl, n_frames, True, cap).cpu().numpy()
        flat = host[n_frames:n_frames + 8 * int(counts.sum())].reshape(-1, 8)
        res, o = [], 0
        for c in counts:
            b = flat[o:o + c, :7].copy()
            o += c
            res.append(b if len(b) else [])
        return res


def _params(cfg, **over):
    p = {k: _get(cfg, k) for k in ("sensor_height", "ground_min_threshold", "ground_min_distance", "cluster_dis",
                                   "cluster_min_points", "discard_max_height", "min_box_volume", "min_box_height",
                                   "max_box_volume", "max_box_len")}
    p["ground_max_threshold"] = 1     # DBSCAN does not pass the config's value: the constructor default applies
    p.update(over)
    return p


class OutlineFitter:
    """outline_utils.py OutlineFitter (l.506-540, 542-958) on the GPU: same constructor arguments and return values."""

    def __init__(self, sensor_height=0, ground_min_threshold=[0.2, -0.2, -0.5], ground_min_distance=[0, 20, 40, 100],
                 ground_max_threshold=1, cluster_dis=0.5, cluster_min_points=40, discard_max_height=4, min_box_volume=0.3,
                 min_box_height=0.5, max_box_volume=200, max_box_len=10, device=None):
        self.sensor_height = sensor_height
        self.ground_min_threshold = ground_min_threshold
        self.ground_min_distance = ground_min_distance
        self.ground_max_threshold = ground_max_threshold
        self.clutter_dis = cluster_dis
        self.clutter_min_points = cluster_min_points
        self.discard_max_height = discard_max_height
        self.min_box_volume = min_box_volume
        self.min_box_hight = min_box_height
        self.max_box_volume = max_box_volume
        self.max_box_len = max_box_len
        self.gpu = OutlineGPU(dict(sensor_height=sensor_height, ground_min_threshold=ground_min_threshold,
                                   ground_min_distance=ground_min_distance, ground_max_threshold=ground_max_threshold,
                                   cluster_dis=cluster_dis, cluster_min_points=cluster_min_points,
                                   discard_max_height=discard_max_height, min_box_volume=min_box_volume,
                                   min_box_height=min_box_height, max_box_volume=max_box_volume, max_box_len=max_box_len),
                              device)

    def compute_volume(self, boxes):
        return np.multiply(np.multiply(boxes[:, 3], boxes[:, 4]), boxes[:, 5])

    def remove_ground(self, points, return_index=False):
        """Non-ground points [M, 3] float64 in the canonical order (and their source rows)."""
        g = self.gpu
        pts, off, _ = g.upload([points])
        xyz, src, cnt, err = g.ground(pts, off, 1)
        n = int(cnt.item())
        if int(err.item()):
            raise _lib.CpdHipError("cpd_outline_ground: segment index outside the table")
        out = xyz[:n].cpu().numpy().astype(np.float64)
        return (out, src[:n].cpu().numpy().astype(np.int64)) if return_index else out

    def _labels(self, points):
        xyz = torch.from_numpy(_exact_f32(points)).to(self.gpu.device)
        n = xyz.shape[0]
        off = torch.tensor([0, n], dtype=torch.int32, device=self.gpu.device)
        cnt = torch.tensor([n], dtype=torch.int32, device=self.gpu.device)
        if n == 0:
            xyz = torch.zeros((1, 3), dtype=torch.float32, device=self.gpu.device)
        labels, ncl = self.gpu.dbscan(xyz, off, cnt, 1)
        return labels[:n].cpu().numpy().astype(np.int64), int(ncl.item())

    def clustering(self, points):
        points = np.asarray(points)
        labels, ncl = self._labels(points)
        self.labels_ = labels
        clusters, labs = [], []
        for i in range(ncl):
            m = labels == i
            this = points[m]
            if len(this) > self.clutter_min_points and this[:, 2].max() < self.discard_max_height:
                clusters.append(this)
                labs.append(labels[m])
        return clusters, labs

    def box_fit(self, points_list, offset=0.2):
        if offset != 0.2:
            raise NotImplementedError("cpd_amd.outline: box_fit's offset is fixed at 0.2 in the kernel")
        if len(points_list) == 0:
            return []
        g = self.gpu
        points_list = [p for p in points_list if len(p)]   # an empty cluster raises in the reference: skipped
        if not points_list:
            return []
        xyz = np.concatenate([_exact_f32(p) for p in points_list], 0)
        lab = np.concatenate([np.full(len(p), i, np.int32) for i, p in enumerate(points_list)])
        n = len(xyz)
        dev = g.device
        t_xyz = torch.from_numpy(xyz).to(dev)
        off = torch.tensor([0, n], dtype=torch.int32, device=dev)
        cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        out = g.boxes(t_xyz, off, cnt, torch.from_numpy(lab).to(dev), torch.tensor([len(points_list)], dtype=torch.int32,
                                                                                  device=dev), 1, False, len(points_list))
        host = out.cpu().numpy()
        k = int(host[0])
        boxes = host[1:1 + 8 * k].reshape(-1, 8)[:, :7].copy()
        return boxes if k else []

    def get_box_cls(self, boxes, config, return_name=True):
        boxes, cls, dif = get_box_cls(boxes, config)
        if not return_name and len(cls):
            proto = _get(config, "cls")
            cls = np.array([proto[c] for c in cls])
        return boxes, cls, dif

    def __call__(self, points):
        return self.gpu.frames_boxes([points])[0]


def outline_frames(frames, generator_cfg, device=None, chunk=16, gpu=None):
    """Per frame (outline_box, outline_cls, outline_dif) as DBSCAN.generate_outline_box stores them: one set of launches and
    one read-back per chunk of frames."""
    gpu = gpu or OutlineGPU(_params(generator_cfg), device)
    res = []
    for c0, c1 in dtype_runs(frames, chunk):
        for boxes in gpu.frames_boxes(frames[c0:c1]):
            b, cls, dif = get_box_cls(boxes, generator_cfg)
            b, cls, _, dif, _, _ = drop_cls(b, cls, dif=dif)
            res.append((b, cls, dif))
    return res


def _paths(seq_name, root_path, method):
    return (os.path.join(root_path, seq_name, seq_name + '.pkl'),
            os.path.join(root_path, seq_name, seq_name + '_outline_' + str(method) + '.pkl'))


class DBSCAN:
    """dbscan.py DBSCAN: the same file contract (<seq>/<seq>.pkl in, <seq>/<seq>_outline_DBSCAN.pkl out, cached)."""

    def __init__(self, seq_name, root_path, config, device=None, chunk=16):
        self.seq_name, self.root_path, self.dataset_cfg = seq_name, root_path, config
        self.chunk = chunk
        self.gpu = OutlineGPU(_params(_get(config, "GeneratorConfig")), device)

    def generate_outline_box(self):
        method = _get(self.dataset_cfg, "InitLabelGenerator")
        in_pkl, out_pkl = _paths(self.seq_name, self.root_path, method)
        if os.path.exists(out_pkl):
            with open(out_pkl, 'rb') as f:
                return pkl.load(f)
        with open(in_pkl, 'rb') as f:
            infos = pkl.load(f)
        gcfg = _get(self.dataset_cfg, "GeneratorConfig")
        paths = [frame_path(os.path.join(self.root_path, self.seq_name), i) for i in range(len(infos))]
        for idx, frames in prefetched_chunks(paths, self.chunk):   # the next chunk's reads overlap this chunk's kernels
            for i, (b, cls, dif) in zip(idx, outline_frames(frames, gcfg, chunk=self.chunk, gpu=self.gpu)):
                infos[i]['outline_box'], infos[i]['outline_cls'], infos[i]['outline_dif'] = b, cls, dif
        with open(out_pkl, 'wb') as f:
            pkl.dump(infos, f)
        return infos

    def __call__(self):
        return self.generate_outline_box()


all_init = {'DBSCAN': DBSCAN}


def compute_outline_box(seq_name, root_path, dataset_cfg):
    """cpd/unsupervised_core/__init__.py compute_outline_box for InitLabelGenerator 'DBSCAN'; every LabelRefiner is refused."""
    return dispatch_outline_box(seq_name, root_path, dataset_cfg, all_init, (), "outline")


def create_outline_boxes(seq_names, root_path, dataset_cfg, device=None, chunk=16):
    """Single-process sequence driver: every sequence through one GPU context (the dataset's Pool(16) of forked workers must
    not each open the GPU); .npy reads run on a small thread pool while the GPU works."""
    return [compute_outline_box(s, root_path, dataset_cfg) for s in seq_names]
