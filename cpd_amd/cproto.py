"""GPU drop-in for the first stage of CPD's C_PROTO refiner (cpd/unsupervised_core/c_proto_refine.py): CSS, C_PROTO.
compute_css_score_and_raw_proto and construct_prototypes, with outline_utils.py's smooth_points, compute_confidence,
hierarchical_occupancy_score and KL_entropy_score. For every box of a chunk of frames the radius crop, the density filter, the
height window, ground removal, DBSCAN, the choice of the largest valid cluster and the occupancy cell counts run as HIP kernels
(csrc/cproto.hip, csrc/outline.hip) on SEGMENTS -- one (frame, box) pair each; the score formula, the prototype ids, the rigid
transforms of a repeated prototype and construct_prototypes are the reference's numpy on the host.

Exactness contract: masks, z_min, new_box, the non-ground rows and their order, DBSCAN labels and the chosen
cluster are the reference's (with ground_removal's argsort stable: the canonical order of DESIGN §5l). The cell counts are those
of the closed-form float32 inverse of the box transform and the unfused float64 product (the reference leaves both to LAPACK /
BLAS), which differ from the reference's on a few per cent of the boxes by one cell.

Not provided here: refine_box_size, refine_box_pos and C_PROTO.__call__ (they need correct_orientation and density_guided_drift):
cpd_amd.cproto_refine's C_PROTO, a subclass of this one, has them.
"""
import copy
import ctypes
import os
import pickle as pkl

import numpy as np

from .seq_io import _get, dtype_runs, frame_path, gpu_modules, prefetched_chunks, run_sequences

# GeneratorConfig / RefinerConfig of tools/cfgs/dataset_configs/waymo_unsupervised/waymo_unsupervised_cproto.yaml (the keys the
# first stage reads)
CPROTO_CONFIG = dict(
    InitLabelGenerator='MFCF', LabelRefiner='C_PROTO',
    GeneratorConfig=dict(sensor_height=0, ground_min_threshold=[0.2, -0.5, -0.5], ground_min_distance=[0, 20, 40, 100],
                         ground_max_threshold=1, cluster_dis=0.5, cluster_min_points=5, discard_max_height=4,
                         min_box_volume=0.1, min_box_height=0.3, max_box_volume=200, max_box_len=10),
    RefinerConfig=dict(GroundMin=[-0.5, -1, -1.5],
                       CSSConfig=dict(MaxDis=80, MLOParts=[9, 7, 5],
                                      PredifinedSize={'Vehicle': [5.065, 1.86, 1.49], 'Pedestrian': [1.0, 1.0, 2.0],
                                                      'Cyclist': [1.9, 0.85, 1.8]},
                                      CSS_weight=[1, 1, 1]),
                       BasicProtoScoreThresh={'Vehicle': 0.8, 'Pedestrian': 0.7, 'Cyclist': 0.7},
                       HighQualityMotionThresh=0.5, HighQualityProtoNum={'Vehicle': 10, 'Pedestrian': 5, 'Cyclist': 5}))

CLASSES = ('Vehicle', 'Pedestrian', 'Cyclist')
# Segments per launch sequence. cpd_outline_ground's workspace holds 152 x 150 cells x 36 bytes = 0.82 MB per segment
# (cpd_outline_ground_workspace_bytes) and cpd_outline_dbscan takes at most 1023 frames (one of them is the tail segment of
# cpd_cproto_filter): 128 segments keep the ground workspace at 106 MB.
SUB_BATCH = 128
MAX_PARTS, MAX_PART = 4, 16      # cproto.hip CP_MAX_PARTS, CP_MAX_PART


def KL_entropy_score(x, y, max_dif=0.05):
    """outline_utils.py:25-32 (host)."""
    KL = 0.0
    for i in range(len(x)):
        KL += x[i] * np.log(x[i] / y[i])
    if KL > max_dif:
        KL = max_dif
    return (max_dif - KL) / max_dif


def points_rigid_transform(cloud, pose):
    """outline_utils.py:328-338 (host): [N, 3] float32 through the float64 matrix product."""
    cloud = np.array(cloud)
    if cloud.shape[0] == 0:
        return cloud
    mat = np.ones(shape=(cloud.shape[0], 4), dtype=np.float32)
    mat[:, 0:3] = cloud[:, 0:3]
    T = np.array((np.asarray(pose) @ mat.astype(np.float64).T).T, dtype=np.float32)
    return T[:, 0:3]


def inverse_box_rows(boxes):
    """Rows 0 and 1 of the inverse of compute_confidence's float32 trans_mat (l.405-414) for boxes [S, 7]: the closed form in
    float64 over the float32 entries (cos yaw, sin yaw, x, y), divided by c*c + s*s, rounded to float32 -> [S, 8]."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    c = np.cos(boxes[:, 6]).astype(np.float32).astype(np.float64)
    s = np.sin(boxes[:, 6]).astype(np.float32).astype(np.float64)
    x = boxes[:, 0].astype(np.float32).astype(np.float64)
    y = boxes[:, 1].astype(np.float32).astype(np.float64)
    d = c * c + s * s
    z = np.zeros_like(c)
    m = np.stack([c / d, s / d, z, -(c * x + s * y) / d, -s / d, c / d, z, (s * x - c * y) / d], -1)
    return np.ascontiguousarray(m.astype(np.float32))


class CProtoGPU:
    """The launch sequence of the first stage on one device. Frames go in as [N_i, >=3] float16 / float32 arrays of one
    dtype, segments as boxes [S, 7] float64 (after the size overwrite) with the frame each belongs to."""

    def __init__(self, config=None, device=None, sub_batch=SUB_BATCH):
        from . import outline
        config = CPROTO_CONFIG if config is None else config
        gcfg, rcfg = _get(config, "GeneratorConfig"), _get(config, "RefinerConfig")
        params = outline._params(gcfg, ground_min_threshold=list(_get(rcfg, "GroundMin")))
        self.ol = outline.OutlineGPU(params, device)
        self.device = self.ol.device
        self.ws = self.ol.ws
        self.cluster_min_points = int(params["cluster_min_points"])
        self.discard_max_height = float(params["discard_max_height"])
        self.set_parts(list(_get(_get(rcfg, "CSSConfig"), "MLOParts")))
        if not 1 <= int(sub_batch) <= 1022:
            raise ValueError("cpd_amd.cproto: sub_batch must be 1..1022 segments")
        self.sub_batch = int(sub_batch)

    def set_parts(self, parts):
        parts = [int(p) for p in parts]
        if not 1 <= len(parts) <= MAX_PARTS or any(p < 1 or p > MAX_PART for p in parts):
            raise NotImplementedError("cpd_amd.cproto: MLOParts holds 1..%d values of 1..%d (got %r)" % (MAX_PARTS, MAX_PART, parts))
        self.parts = parts
        self.c_parts = (ctypes.c_int32 * len(parts))(*parts)

    def upload(self, frames):
        return self.ol.upload(frames)

    # -- stages (device tensors in, device tensors out) --
    def crop(self, pts, off, n_frames, boxes, seg_frame):
        torch, _lib = gpu_modules()
        lib, S, dev = _lib.lib(), int(boxes.shape[0]), self.device
        is_half = 1 if pts.dtype == torch.float16 else 0
        seg_off = torch.empty(S + 1, dtype=torch.int32, device=dev)
        nb = lib.cpd_cproto_crop_workspace_bytes(S)
        ws = self.ws.get("cproto_crop", nb)
        head = (_lib.ptr(pts), is_half, int(pts.stride(0)) if pts.shape[0] else 3, _lib.ptr(off), n_frames, _lib.ptr(boxes),
                _lib.ptr(seg_frame), S)
        _lib.check(lib.cpd_cproto_crop_count(*head, _lib.ptr(seg_off), _lib.ptr(ws), nb, _lib.stream()), "cpd_cproto_crop_count")
        n_rows = int(seg_off[S].item())      # the one read-back before the results: sizes every buffer below
        rows = torch.empty((max(n_rows, 1), 3), dtype=pts.dtype, device=dev)
        src = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.cpd_cproto_crop_fill(*head, _lib.ptr(seg_off), n_rows, _lib.ptr(rows), _lib.ptr(src), _lib.stream()),
                   "cpd_cproto_crop_fill")
        return rows, src, seg_off, n_rows

    def filter(self, rows, src, seg_off, boxes, n_rows, radius=0.2):
        torch, _lib = gpu_modules()
        lib, S, dev = _lib.lib(), int(boxes.shape[0]), self.device
        out = dict(dens_mask=torch.empty(max(n_rows, 1), dtype=torch.uint8, device=dev),
                   z_min=torch.empty(max(S, 1), dtype=torch.float64, device=dev),
                   new_box=torch.empty((max(S, 1), 7), dtype=torch.float64, device=dev),
                   had_points=torch.empty(max(S, 1), dtype=torch.int32, device=dev),
                   filt_rows=torch.empty((max(n_rows, 1), 3), dtype=rows.dtype, device=dev),
                   filt_src=torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev),
                   filt_off=torch.empty(S + 2, dtype=torch.int32, device=dev))
        nb = lib.cpd_cproto_filter_workspace_bytes(S, n_rows)
        ws = self.ws.get("cproto_filter", nb)
        _lib.check(lib.cpd_cproto_filter(_lib.ptr(rows), 1 if rows.dtype == torch.float16 else 0, _lib.ptr(seg_off),
                                         _lib.ptr(src), _lib.ptr(boxes), S, n_rows, float(radius), _lib.ptr(out["dens_mask"]),
                                         _lib.ptr(out["z_min"]), _lib.ptr(out["new_box"]), _lib.ptr(out["had_points"]),
                                         _lib.ptr(out["filt_rows"]), _lib.ptr(out["filt_src"]), _lib.ptr(out["filt_off"]),
                                         _lib.ptr(ws), nb, _lib.stream()), "cpd_cproto_filter")
        return out

    def score(self, xyz, ng_src, off, cnt, labels, ncl, had, filt_src, m, new_box, S, n_rows, min_rows=10,
              cluster_min_points=None, discard_max_height=None):
        torch, _lib = gpu_modules()
        lib, dev = _lib.lib(), self.device
        P = len(self.parts)
        out = dict(occ=torch.empty((max(S, 1), P), dtype=torch.int32, device=dev),
                   best_label=torch.empty(max(S, 1), dtype=torch.int32, device=dev),
                   best_count=torch.empty(max(S, 1), dtype=torch.int32, device=dev),
                   out_off=torch.empty(S + 1, dtype=torch.int32, device=dev),
                   out_xyz=torch.empty((max(n_rows, 1), 3), dtype=torch.float32, device=dev),
                   out_src=torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev))
        nb = lib.cpd_cproto_score_workspace_bytes(S, n_rows)
        ws = self.ws.get("cproto_score", nb)
        _lib.check(lib.cpd_cproto_score(
            _lib.ptr(xyz), _lib.ptr(ng_src), _lib.ptr(off), _lib.ptr(cnt), _lib.ptr(labels), _lib.ptr(ncl), _lib.ptr(had),
            _lib.ptr(filt_src), _lib.ptr(m), _lib.ptr(new_box), S, n_rows, self.c_parts, P, int(min_rows),
            int(self.cluster_min_points if cluster_min_points is None else cluster_min_points),
            float(self.discard_max_height if discard_max_height is None else discard_max_height), _lib.ptr(out["occ"]),
            _lib.ptr(out["best_label"]), _lib.ptr(out["best_count"]), _lib.ptr(out["out_off"]), _lib.ptr(out["out_xyz"]),
            _lib.ptr(out["out_src"]), _lib.ptr(ws), nb, _lib.stream()), "cpd_cproto_score")
        return out

    # -- one sub-batch: every launch, then one copy back --
    def _run_sub(self, pts, off, n_frames, boxes, seg_frame, stages):
        torch, _lib = gpu_modules()
        dev = self.device
        S = len(boxes)
        d_boxes = torch.from_numpy(np.ascontiguousarray(boxes, np.float64)).to(dev)
        d_segf = torch.from_numpy(np.ascontiguousarray(seg_frame, np.int32)).to(dev)
        d_m = torch.from_numpy(inverse_box_rows(boxes)).to(dev)
        rows, src, seg_off, n_rows = self.crop(pts, off, n_frames, d_boxes, d_segf)
        f = self.filter(rows, src, seg_off, d_boxes, n_rows)
        xyz, ng_src, cnt, err = self.ol.ground(f["filt_rows"][:n_rows], f["filt_off"], S + 1)
        labels, ncl = self.ol.dbscan(xyz, f["filt_off"], cnt, S + 1)
        sc = self.score(xyz, ng_src, f["filt_off"], cnt, labels, ncl, f["had_points"], f["filt_src"], d_m, f["new_box"], S,
                        n_rows)
        back = [("z_min", f["z_min"]), ("new_box", f["new_box"]), ("had_points", f["had_points"]), ("occ", sc["occ"]),
                ("best_label", sc["best_label"]), ("best_count", sc["best_count"]), ("out_off", sc["out_off"]), ("err", err),
                ("out_xyz", sc["out_xyz"]), ("out_src", sc["out_src"])]
        if stages:
            back += [("seg_off", seg_off), ("crop_src", src), ("dens_mask", f["dens_mask"]), ("filt_off", f["filt_off"]),
                     ("filt_src", f["filt_src"]), ("ng_count", cnt), ("ng_src", ng_src), ("labels", labels)]
        res = _copy_back(back)
        if int(res["err"][0]):
            raise _lib.CpdHipError("cpd_outline_ground: segment index outside the table")
        oo = res["out_off"]
        out = dict(z_min=res["z_min"][:S], new_box=res["new_box"][:S], had_points=res["had_points"][:S].astype(bool),
                   occ=res["occ"][:S], best_label=res["best_label"][:S], best_count=res["best_count"][:S],
                   cluster=[res["out_xyz"][oo[s]:oo[s + 1]].astype(np.float64) for s in range(S)],
                   cluster_src=[res["out_src"][oo[s]:oo[s + 1]].astype(np.int64) for s in range(S)])
        if stages:
            so, fo = res["seg_off"], res["filt_off"]
            out["crop_src"] = [res["crop_src"][so[s]:so[s + 1]].astype(np.int64) for s in range(S)]
            out["dens_mask"] = [res["dens_mask"][so[s]:so[s + 1]].astype(bool) for s in range(S)]
            out["filt_src"] = [res["filt_src"][fo[s]:fo[s + 1]].astype(np.int64) for s in range(S)]
            out["ng_src"] = [out["filt_src"][s][res["ng_src"][fo[s]:fo[s] + res["ng_count"][s]]] for s in range(S)]
            # the reference clusters only where more than 10 non-ground rows are left
            out["labels"] = [res["labels"][fo[s]:fo[s] + (res["ng_count"][s] if res["ng_count"][s] > 10 else 0)].astype(np.int64)
                             for s in range(S)]
        return out

    def run(self, frames, boxes, seg_frame, stages=False):
        """frames: list of [N, >=3] arrays of one dtype (or the tuple upload() returned); boxes [S, 7]; seg_frame [S]. Returns a
        dict of host arrays / per-segment lists: z_min, new_box, had_points, occ [S, P], best_label, best_count, cluster (the
        chosen cluster's rows, float64), cluster_src (their rows in the frame); with stages also crop_src, dens_mask, filt_src,
        ng_src and labels per segment."""
        pts, off, off_host = frames if isinstance(frames, tuple) else self.upload(frames)
        n_frames = len(off_host) - 1
        boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
        seg_frame = np.asarray(seg_frame, np.int32).reshape(-1)
        if len(seg_frame) != len(boxes) or (len(boxes) and (seg_frame.min() < 0 or seg_frame.max() >= n_frames)):
            raise ValueError("cpd_amd.cproto: one frame index in 0..%d per box" % (n_frames - 1))
        parts = [self._run_sub(pts, off, n_frames, boxes[s:s + self.sub_batch], seg_frame[s:s + self.sub_batch], stages)
                 for s in range(0, len(boxes), self.sub_batch)]
        if not parts:
            parts = [self._run_sub(pts, off, n_frames, boxes, seg_frame, stages)]
        out = {}
        for k in parts[0]:
            vals = [p[k] for p in parts]
            out[k] = sum(vals, []) if isinstance(vals[0], list) else np.concatenate(vals, 0)
        return out


def _copy_back(back):
    """[(name, device tensor)] -> {name: host array} through one device-to-host copy."""
    torch, _ = gpu_modules()
    host = torch.cat([t.reshape(-1).view(torch.uint8) for _, t in back]).cpu().numpy()
    res, o = {}, 0
    for name, t in back:
        nbytes = t.numel() * t.element_size()
        res[name] = host[o:o + nbytes].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape))
        o += nbytes
    return res


_GPU = {}


def _gpu(device=None):
    torch, _ = gpu_modules()
    dev = torch.device(device if device is not None else "cuda")
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    g = _GPU.get(key)
    if g is None:
        g = _GPU[key] = CProtoGPU(CPROTO_CONFIG, dev)
    return g


def _device_points(points):
    """[N, >=3] float16 / float32 rows as they are; wider floats must hold float32 values."""
    points = np.asarray(points)
    if points.dtype in (np.float16, np.float32):
        return points
    f = points[:, 0:3].astype(np.float32)
    if not np.array_equal(f.astype(np.float64), np.asarray(points[:, 0:3], np.float64)):
        raise ValueError("cpd_amd.cproto: coordinates must be float16 / float32 values")
    return f


def smooth_points(points, rad=0.2, device=None):
    """outline_utils.py:391-396 on the GPU: the rows with more than 3 rows (itself included) within rad."""
    torch, _ = gpu_modules()
    points = np.asarray(points)
    n = len(points)
    if n == 0:
        return points
    g = _gpu(device)
    rows = torch.from_numpy(np.ascontiguousarray(_device_points(points)[:, 0:3])).to(g.device)
    src = torch.arange(n, dtype=torch.int32, device=g.device)
    seg_off = torch.tensor([0, n], dtype=torch.int32, device=g.device)
    box = torch.zeros((1, 7), dtype=torch.float64, device=g.device)
    mask = g.filter(rows, src, seg_off, box, n, rad)["dens_mask"][:n].cpu().numpy().astype(bool)
    return points[mask]


def _occupancy(points, box, parts, device=None):
    torch, _ = gpu_modules()
    g = _gpu(device)
    pts = np.ascontiguousarray(_device_points(np.asarray(points))[:, 0:3].astype(np.float32))
    n, dev = len(pts), g.device
    box = np.asarray(box, np.float64).reshape(1, 7)
    keep = g.parts
    g.set_parts(parts)
    try:
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        xyz = torch.from_numpy(pts).to(dev) if n else torch.zeros((1, 3), dtype=torch.float32, device=dev)
        idx = torch.arange(max(n, 1), dtype=torch.int32, device=dev)
        sc = g.score(xyz, idx, i32([0, n, n]), i32([n, 0]), torch.zeros(max(n, 1), dtype=torch.int32, device=dev), i32([1, 0]),
                     i32([1, 0]), idx, torch.from_numpy(inverse_box_rows(box)).to(dev), torch.from_numpy(box).to(dev), 1, n,
                     min_rows=-1, cluster_min_points=0, discard_max_height=float("inf"))
        return sc["occ"][0].cpu().numpy()
    finally:
        g.set_parts(keep)


def compute_confidence(points, box, parts=6, device=None):
    """outline_utils.py:398-436: the share of the parts x parts cells of the box that hold more than one point."""
    return int(_occupancy(points, box, [parts], device)[0]) / (parts ** 2)


def hierarchical_occupancy_score(points, box, parts=[7, 5, 3], device=None):
    """outline_utils.py:438-442, the cell counts of all `parts` from one launch."""
    occ = _occupancy(points, box, list(parts), device)
    all_confi = 0
    for o, part in zip(occ, parts):
        all_confi += int(o) / (part ** 2)
    return all_confi / len(parts)


class CSS():
    """c_proto_refine.py:13-44; only the occupancy counts come from the device."""

    def __init__(self, config):
        self.max_dis = _get(config, "MaxDis")
        self.mlo_parts = _get(config, "MLOParts")
        self.predifined_size = _get(config, "PredifinedSize")
        self.weights = np.array(_get(config, "CSS_weight"))

    def dis_score(self, box):
        dis_dis = np.linalg.norm(box[0:3])
        if dis_dis > self.max_dis:
            dis_dis = self.max_dis
        return 1 - dis_dis / self.max_dis

    def mlo_score(self, occ):
        all_confi = 0
        for o, part in zip(occ, self.mlo_parts):
            all_confi += int(o) / (part ** 2)
        return all_confi / len(self.mlo_parts)

    def size_score(self, box, name):
        new_box = copy.deepcopy(box)
        this_size_norm = new_box[3:6] / new_box[3:6].sum()
        this_temp_norm = np.array(self.predifined_size[name])
        this_temp_norm = this_temp_norm / this_temp_norm.sum()
        return KL_entropy_score(this_size_norm, this_temp_norm)

    def from_occ(self, occ, box, name):
        weights = np.array(self.weights) / np.sum(self.weights)
        return self.dis_score(box) * weights[0] + self.mlo_score(occ) * weights[1] + self.size_score(box, name) * weights[2]

    def compute_css(self, points, box, name, device=None):
        box = np.asarray(box, np.float64)
        return self.from_occ(_occupancy(points, box, list(self.mlo_parts), device), box, name)

    def __call__(self, points, box, name):
        return self.compute_css(points, box, name)


class C_PROTO():
    """c_proto_refine.py:46-330: the same files (<seq>_outline_<Init>.pkl in, <seq>_outline_<Init>_CSS.pkl and
    _CSS_raw_proto.pkl out, cached; construct_prototypes: _CSS_proto.pkl)."""

    def __init__(self, seq_name, root_path, config, device=None, chunk=16, sub_batch=SUB_BATCH):
        self.seq_name = seq_name
        self.root_path = root_path
        self.dataset_cfg = config
        self.device, self.chunk, self.sub_batch = device, chunk, sub_batch
        self.css_estimator = CSS(_get(_get(config, "RefinerConfig"), "CSSConfig"))
        self._gpu = None

    @property
    def gpu(self):
        if self._gpu is None:
            self._gpu = CProtoGPU(self.dataset_cfg, self.device, self.sub_batch)
        return self._gpu

    def _path(self, suffix):
        init = str(_get(self.dataset_cfg, "InitLabelGenerator"))
        return os.path.join(self.root_path, self.seq_name, self.seq_name + '_outline_' + init + suffix + '.pkl')

    def frame_chunks(self, n):
        """(indices, frames) per chunk of the sequence's n frame files; the next chunk's reads overlap this chunk's kernels."""
        seq_dir = os.path.join(self.root_path, self.seq_name)
        return prefetched_chunks([frame_path(seq_dir, i) for i in range(n)], self.chunk)

    def score_frames(self, frames, infos, raw_proto_set, stages=None):
        """l.91-188 for the frames (a list of [N, 3] arrays) that go with infos (updated in place)."""
        css = self.css_estimator
        thresh = _get(_get(self.dataset_cfg, "RefinerConfig"), "BasicProtoScoreThresh")
        seq_id = int(self.seq_name[8:16])
        frames = [np.asarray(f) for f in frames]
        for c0, c1 in dtype_runs(frames, self.chunk):
            boxes, seg_frame, where = [], [], []
            for i in range(c0, c1):     # the size overwrite (l.111-118); classes outside the three are skipped
                for b in range(len(infos[i]['outline_box'])):
                    name = infos[i]['outline_cls'][b]
                    if name not in raw_proto_set:
                        continue
                    this_box = infos[i]['outline_box'][b]
                    if name == 'Pedestrian':
                        this_box[3:5] = np.array(css.predifined_size['Pedestrian'])[0:2]
                    if name == 'Cyclist':
                        this_box[4] = np.array(css.predifined_size['Cyclist'])[1]
                    infos[i]['outline_box'][b] = this_box
                    boxes.append(np.array(this_box, np.float64))
                    seg_frame.append(i - c0)
                    where.append((i, b))
            res = self.gpu.run(frames[c0:c1], np.array(boxes).reshape(-1, 7), seg_frame, stages is not None)
            if stages is not None:
                stages.append((where, res))
            scores = {i: np.zeros(shape=infos[i]['outline_cls'].shape) for i in range(c0, c1)}
            for s, (i, b) in enumerate(where):
                if res["best_label"][s] < 0:
                    continue
                name, pose = infos[i]['outline_cls'][b], infos[i]['pose']
                new_box = np.array(res["new_box"][s])
                max_cluter = res["cluster"][s]
                css_score = css.from_occ(res["occ"][s], new_box, name)
                scores[i][b] = css_score
                infos[i]['outline_box'][b] = new_box
                if css_score > thresh[name]:
                    proto_id = int(str(seq_id) + str(infos[i]['outline_ids'][b]))
                    global_position = points_rigid_transform([new_box[0:3]], pose)[0:, 0:3]
                    if proto_id in raw_proto_set[name]:
                        e = raw_proto_set[name][proto_id]
                        pose_i = np.linalg.inv(e['pose'][0])
                        max_cluter_global = points_rigid_transform(max_cluter, pose)
                        e['points'].append(points_rigid_transform(max_cluter_global, pose_i))
                        e['outline_box'].append(new_box)
                        e['pose'].append(pose)
                        e['score'].append(css_score)
                        e['global_position'].append(global_position)
                    else:
                        raw_proto_set[name][proto_id] = {'points': [max_cluter], 'outline_box': [new_box], 'pose': [pose],
                                                         'score': [css_score], 'global_position': [global_position]}
            for i in range(c0, c1):
                infos[i]['outline_score'] = scores[i]

    def compute_css_score_and_raw_proto(self):
        output_pkl_path, output_raw_proto_path = self._path('_CSS'), self._path('_CSS_raw_proto')
        raw_proto_set = {c: {} for c in CLASSES}
        if os.path.exists(output_pkl_path):
            with open(output_pkl_path, 'rb') as f:
                return pkl.load(f)
        with open(self._path(''), 'rb') as f:
            outline_infos = pkl.load(f)
        for idx, frames in self.frame_chunks(len(outline_infos)):
            self.score_frames(frames, outline_infos[idx[0]:idx[0] + len(frames)], raw_proto_set)
        with open(output_pkl_path, 'wb') as f:
            pkl.dump(outline_infos, f)
        with open(output_raw_proto_path, 'wb') as f:
            pkl.dump(raw_proto_set, f)
        return outline_infos

    def limit(self, ang):
        return _limit(ang)

    def construct_prototypes(self):
        """l.207-330: basic_proto_set, high_quality_proto_set and proto_points_set from the raw-proto file (host only)."""
        output_proto_info_path = self._path('_CSS_proto')
        if os.path.exists(output_proto_info_path):
            with open(output_proto_info_path, 'rb') as f:
                return pkl.load(f)
        with open(self._path('_CSS_raw_proto'), 'rb') as f:
            raw_proto_set = pkl.load(f)
        proto_set = construct_prototypes(raw_proto_set, _get(self.dataset_cfg, "RefinerConfig"))
        with open(output_proto_info_path, 'wb') as f:
            pkl.dump(proto_set, f)
        return proto_set

    def refine_box_size(self):
        raise NotImplementedError("cpd_amd.cproto: refine_box_size has no GPU drop-in yet (it needs correct_orientation and "
                                  "density_guided_drift)")

    def refine_box_pos(self):
        raise NotImplementedError("cpd_amd.cproto: refine_box_pos has no GPU drop-in yet (it follows refine_box_size, which "
                                  "needs correct_orientation and density_guided_drift)")

    def __call__(self):
        raise NotImplementedError("cpd_amd.cproto: the whole refiner is not provided (refine_box_size needs correct_orientation "
                                  "and density_guided_drift); call compute_css_score_and_raw_proto and construct_prototypes")


def _limit(ang):
    """C_PROTO.limit (l.197-204)."""
    ang = ang % (2 * np.pi)
    ang[ang > np.pi] = ang[ang > np.pi] - 2 * np.pi
    ang[ang < -np.pi] = ang[ang < -np.pi] + 2 * np.pi
    return ang


def construct_prototypes(raw_proto_set, refiner_cfg):
    """The body of C_PROTO.construct_prototypes (l.227-325) over a loaded raw_proto_set."""
    limit = _limit
    high_quality_motion_thresh = _get(refiner_cfg, "HighQualityMotionThresh")
    high_quality_proto_num = _get(refiner_cfg, "HighQualityProtoNum")
    basic_proto_set = {c: {} for c in CLASSES}
    high_quality_proto_set = {c: {} for c in CLASSES}
    proto_points_set = {c: {} for c in CLASSES}
    for cls_name in raw_proto_set.keys():
        id_list, score_list, points_set_list, box_list = [], [], [], []
        for proto_id in raw_proto_set[cls_name].keys():
            all_points = raw_proto_set[cls_name][proto_id]['points']
            box_set = np.array(raw_proto_set[cls_name][proto_id]['outline_box'])
            pose_set = raw_proto_set[cls_name][proto_id]['pose']
            global_position_set = np.array(raw_proto_set[cls_name][proto_id]['global_position'])
            score_set = raw_proto_set[cls_name][proto_id]['score']
            score_mean = np.mean(score_set)
            mean_position = np.mean(global_position_set[:, 0:2], 0)
            position_dis = global_position_set[:, 0:2] - mean_position
            dis = np.linalg.norm(position_dis, axis=1)
            std = np.std(dis)
            whl_mean = np.mean(box_set[:, 3:6], 0)
            basic_proto_set[cls_name][proto_id] = whl_mean
            if std <= high_quality_motion_thresh:
                points_set = np.concatenate(all_points, 0)
                id_list.append(proto_id)
                score_list.append(-score_mean)
                points_set_list.append(points_set)
                mean_box = copy.deepcopy(box_set[0])
                mean_box[3:6] = whl_mean
                pose_i = np.linalg.inv(pose_set[0])
                new_mean_position = points_rigid_transform([mean_position], pose_i)[0:, 0:3]
                mean_box[0:3] = new_mean_position
                max_s_arg = np.argmax(score_set)
                angle_max = box_set[max_s_arg, 6]
                angles = box_set[:, 6]
                angles = limit(angles)
                res = angles - angle_max
                res = limit(res)
                res = res[np.abs(res) < 1.5]
                res = res.mean()
                mean_box[6] = angle_max + res
                box_list.append(mean_box)
                proto_points_set[cls_name][proto_id] = {'box': mean_box, 'points': points_set, 'score': score_mean, 'move': 0}
            else:
                arg_max = np.argmax(score_set)
                this_points_set = all_points[arg_max]
                max_score = score_set[arg_max]
                max_box = box_set[arg_max]
                pose_i = np.linalg.inv(pose_set[arg_max])
                this_points_set[:, 0:3] = points_rigid_transform(this_points_set[:, 0:3], pose_set[0])[:, 0:3]
                this_points_set[:, 0:3] = points_rigid_transform(this_points_set[:, 0:3], pose_i)[:, 0:3]
                proto_points_set[cls_name][proto_id] = {'box': max_box, 'points': this_points_set, 'score': max_score, 'move': 1}
        if len(score_list) == 0:
            continue
        arg_max_score = np.argsort(score_list)
        proto_num = min(high_quality_proto_num[cls_name], len(arg_max_score))
        for list_id in arg_max_score[0:proto_num]:
            high_quality_proto_set[cls_name][id_list[list_id]] = {'box': box_list[list_id]}
    return {'basic_proto_set': basic_proto_set, 'high_quality_proto_set': high_quality_proto_set,
            'proto_points_set': proto_points_set}


def create_css(seq_names, root_path, dataset_cfg, device=None, chunk=16):
    """Single-process sequence driver (forked workers must not each open the GPU): every sequence's
    compute_css_score_and_raw_proto and construct_prototypes through one GPU context."""
    def run(c):
        infos = c.compute_css_score_and_raw_proto()
        c.construct_prototypes()
        return infos
    return run_sequences(lambda s: C_PROTO(s, root_path, dataset_cfg, device, chunk), seq_names, run)
