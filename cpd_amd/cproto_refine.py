"""GPU drop-in for the second half of CPD's C_PROTO refiner (cpd/unsupervised_core/c_proto_refine.py:332-683): C_PROTO.
refine_box_size, refine_box_pos and __call__, with outline_utils.py's correct_orientation, density_guided_drift,
angle_from_vector, get_registration_angle and box_rigid_transform. refine_box_size repeats the first stage's per-box work
(cpd_amd.cproto: crop, density filter, height window, ground removal, DBSCAN, cluster choice, cell counts) with the prototype
size fit between the filter and the score and the orientation / drift kernels after it (csrc/cproto_refine.hip); the CSS formula,
the choice between the two drifted boxes and refine_box_pos are the reference's numpy on the host.

Exactness contract: the first stage's (§5n), and for the orientation and the drift the closed-form float32 inverse
of the box transform and unfused float64 products where the reference leaves both to LAPACK / BLAS.

C_PROTO here subclasses cproto.C_PROTO, whose refine_box_size / refine_box_pos / __call__ stay unprovided."""
import copy
import ctypes
import os
import pickle as pkl

import numpy as np

from . import cproto
from .cproto import CLASSES, _copy_back, inverse_box_rows, points_rigid_transform
from .seq_io import _get, dtype_runs, gpu_modules, run_sequences

# RefinerConfig of waymo_unsupervised_cproto.yaml with the two keys the second half reads
REFINE_CONFIG = copy.deepcopy(cproto.CPROTO_CONFIG)
REFINE_CONFIG["RefinerConfig"].update(OrienThresh=0.5, StaticThresh=0.8)

MAX_HQ = 64      # cproto_refine.hip RF_MAX_CAP


class PrototypeTable:
    """What the size fit reads of a _CSS_proto.pkl (l.357-368): the basic prototypes' whl by class and id, and per class the
    high-quality prototypes' ids and whl in the file's insertion order."""

    def __init__(self, proto_set, predefined):
        self.basic = proto_set['basic_proto_set']
        hq = proto_set['high_quality_proto_set']
        self.hq_ids = [list(hq.get(c, {}).keys()) for c in CLASSES]
        self.count = [len(ids) for ids in self.hq_ids]
        if max(self.count) > MAX_HQ:
            raise NotImplementedError("cpd_amd.cproto_refine: at most %d high-quality prototypes per class (got %r)"
                                      % (MAX_HQ, self.count))
        self.cap = max(1, max(self.count))
        self.hq_whl = np.zeros((3, self.cap, 3), np.float64)
        for ci, c in enumerate(CLASSES):
            for k, pid in enumerate(self.hq_ids[ci]):
                self.hq_whl[ci, k] = np.asarray(hq[c][pid]['box'], np.float64)[3:6]
        self.predefined = np.array([predefined[c] for c in CLASSES], np.float64).reshape(3, 3)

    def basic_whl(self, name, proto_id):
        """The NaN row of a box whose own id is no basic prototype."""
        whl = self.basic.get(name, {}).get(proto_id)
        return np.full(3, np.nan) if whl is None else np.asarray(whl, np.float64)[0:3]

    def proto_id(self, ci, fit_index, own_id):
        if fit_index == -2:
            return own_id
        return self.hq_ids[ci][fit_index] if fit_index >= 0 else -1


class RefineGPU(cproto.CProtoGPU):
    """The first stage's launch sequence with the size fit and the orientation / drift kernels: crop, filter, fit_size, ground,
    dbscan, score, orient_drift, one copy back."""

    def set_prototypes(self, table):
        torch, _ = gpu_modules()
        self.table = table
        self.d_hq_whl = torch.from_numpy(table.hq_whl).to(self.device)
        self.c_hq_count = (ctypes.c_int32 * 3)(*table.count)
        self.c_predefined = (ctypes.c_double * 9)(*table.predefined.reshape(-1))

    # -- stages (device tensors in, device tensors out) --
    def fit_size(self, new_box, seg_cls, basic_whl, S):
        """new_box [S, 7] is updated in place; returns fit_index [S]."""
        torch, _lib = gpu_modules()
        fit = torch.empty(max(S, 1), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().cpd_refine_fit_size(_lib.ptr(new_box), _lib.ptr(seg_cls), _lib.ptr(basic_whl), S,
                                                  _lib.ptr(self.d_hq_whl), self.c_hq_count, self.table.cap, self.c_predefined,
                                                  _lib.ptr(fit), _lib.stream()), "cpd_refine_fit_size")
        return fit

    def orient_drift(self, out_xyz, out_off, best_label, new_box, m, S, n_rows):
        torch, _lib = gpu_modules()
        lib, dev = _lib.lib(), self.device
        out = {k: torch.empty((max(S, 1), 7), dtype=torch.float64, device=dev)
               for k in ("box_drift", "box_orient_drift", "box_orient")}
        nb = lib.cpd_refine_orient_drift_workspace_bytes(S)
        ws = self.ws.get("refine_orient", nb)
        _lib.check(lib.cpd_refine_orient_drift(_lib.ptr(out_xyz), _lib.ptr(out_off), _lib.ptr(best_label), _lib.ptr(new_box),
                                               _lib.ptr(m), S, n_rows, _lib.ptr(out["box_drift"]),
                                               _lib.ptr(out["box_orient_drift"]), _lib.ptr(out["box_orient"]), _lib.ptr(ws), nb,
                                               _lib.stream()), "cpd_refine_orient_drift")
        return out

    # -- one sub-batch: every launch, then one copy back --
    def _run_sub(self, pts, off, n_frames, boxes, seg_frame, stages, seg_cls=None, basic_whl=None):
        if seg_cls is None:      # the first stage, unchanged
            return super()._run_sub(pts, off, n_frames, boxes, seg_frame, stages)
        torch, _lib = gpu_modules()
        dev = self.device
        S = len(boxes)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        d_boxes, d_segf = up(boxes, np.float64), up(seg_frame, np.int32)
        d_cls = up(seg_cls, np.int32) if S else torch.zeros(1, dtype=torch.int32, device=dev)
        d_basic = up(basic_whl, np.float64) if S else torch.zeros((1, 3), dtype=torch.float64, device=dev)
        d_m = torch.from_numpy(inverse_box_rows(boxes)).to(dev) if S else torch.zeros((1, 8), dtype=torch.float32, device=dev)
        rows, src, seg_off, n_rows = self.crop(pts, off, n_frames, d_boxes, d_segf)
        f = self.filter(rows, src, seg_off, d_boxes, n_rows)
        fit = self.fit_size(f["new_box"], d_cls, d_basic, S)
        xyz, ng_src, cnt, err = self.ol.ground(f["filt_rows"][:n_rows], f["filt_off"], S + 1)
        labels, ncl = self.ol.dbscan(xyz, f["filt_off"], cnt, S + 1)
        sc = self.score(xyz, ng_src, f["filt_off"], cnt, labels, ncl, f["had_points"], f["filt_src"], d_m, f["new_box"], S,
                        n_rows)
        od = self.orient_drift(sc["out_xyz"], sc["out_off"], sc["best_label"], f["new_box"], d_m, S, n_rows)
        back = [("new_box", f["new_box"]), ("fit_index", fit), ("occ", sc["occ"]), ("best_label", sc["best_label"]),
                ("best_count", sc["best_count"]), ("err", err), ("box_drift", od["box_drift"]),
                ("box_orient_drift", od["box_orient_drift"]), ("box_orient", od["box_orient"])]
        if stages:
            back += [("out_off", sc["out_off"]), ("out_xyz", sc["out_xyz"])]
        res = _copy_back(back)
        if int(res["err"][0]):
            raise _lib.CpdHipError("cpd_outline_ground: segment index outside the table")
        out = {k: res[k][:S] for k in ("new_box", "fit_index", "occ", "best_label", "best_count", "box_drift",
                                       "box_orient_drift", "box_orient")}
        if stages:
            oo = res["out_off"]
            out["cluster"] = [res["out_xyz"][oo[s]:oo[s + 1]].astype(np.float64) for s in range(S)]
        return out

    def run(self, frames, boxes, seg_frame, stages=False, seg_cls=None, basic_whl=None):
        """Without seg_cls: CProtoGPU.run, the first stage. With seg_cls [S] (0 Vehicle, 1 Pedestrian, 2 Cyclist) and basic_whl
        [S, 3] (PrototypeTable.basic_whl): refine_box_size's per-box work; returns host arrays per segment: new_box (fitted),
        fit_index, occ [S, P], best_label, best_count, box_drift, box_orient_drift, box_orient; with stages also cluster (the
        chosen cluster's rows per segment)."""
        if seg_cls is None:
            return super().run(frames, boxes, seg_frame, stages)
        if getattr(self, "table", None) is None:
            raise ValueError("cpd_amd.cproto_refine: set_prototypes() first")
        pts, off, off_host = frames if isinstance(frames, tuple) else self.upload(frames)
        n_frames = len(off_host) - 1
        boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
        seg_frame = np.asarray(seg_frame, np.int32).reshape(-1)
        seg_cls = np.asarray(seg_cls, np.int32).reshape(-1)
        basic_whl = np.asarray(basic_whl, np.float64).reshape(-1, 3)
        if len(seg_frame) != len(boxes) or (len(boxes) and (seg_frame.min() < 0 or seg_frame.max() >= n_frames)):
            raise ValueError("cpd_amd.cproto_refine: one frame index in 0..%d per box" % (n_frames - 1))
        if len(seg_cls) != len(boxes) or len(basic_whl) != len(boxes) or (len(boxes) and (seg_cls.min() < 0 or seg_cls.max() > 2)):
            raise ValueError("cpd_amd.cproto_refine: one class 0..2 and one basic_whl row per box")
        step = self.sub_batch
        parts = [self._run_sub(pts, off, n_frames, boxes[s:s + step], seg_frame[s:s + step], stages, seg_cls[s:s + step],
                               basic_whl[s:s + step]) for s in range(0, max(len(boxes), 1), step)]
        out = {}
        for k in parts[0]:
            vals = [p[k] for p in parts]
            out[k] = sum(vals, []) if isinstance(vals[0], list) else np.concatenate(vals, 0)
        return out


# ---- the two functions on one cluster (reference signatures) --------------------------------------------------------------------

def _orient_drift_one(points, box, device=None):
    torch, _ = gpu_modules()
    g = _gpu(device)
    pts = np.ascontiguousarray(cproto._device_points(np.asarray(points))[:, 0:3].astype(np.float32))
    box = np.asarray(box, np.float64).reshape(1, 7)
    n, dev = len(pts), g.device
    if n == 0:
        raise ValueError("cpd_amd.cproto_refine: an empty cluster has no extent")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    od = g.orient_drift(torch.from_numpy(pts).to(dev), i32([0, n]), i32([0]), torch.from_numpy(box).to(dev),
                        torch.from_numpy(inverse_box_rows(box)).to(dev), 1, n)
    return {k: v[0].cpu().numpy() for k, v in od.items()}


def correct_orientation(points, box, device=None):
    """outline_utils.py:127-326 for one cluster [N, >=3] and one box [7]."""
    return _orient_drift_one(points, box, device)["box_orient"]


def density_guided_drift(points, box, device=None):
    """outline_utils.py:41-92 for one cluster [N, >=3] and one box [7]."""
    return _orient_drift_one(points, box, device)["box_drift"]


_GPU = {}


def _gpu(device=None):
    torch, _ = gpu_modules()
    dev = torch.device(device if device is not None else "cuda")
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    g = _GPU.get(key)
    if g is None:
        g = _GPU[key] = RefineGPU(REFINE_CONFIG, dev)
    return g


# ---- host helpers (outline_utils.py:34-39, 340-366) -----------------------------------------------------------------------------

def angle_from_vector(x, y):
    if x > 0:
        return np.arctan(y / x)
    else:
        return np.pi + np.arctan(y / x)


def get_registration_angle(mat):
    cos_theta = mat[0, 0]
    sin_theta = mat[1, 0]
    if cos_theta < -1:
        cos_theta = -1
    if cos_theta > 1:
        cos_theta = 1
    theta_cos = np.arccos(cos_theta)
    if sin_theta >= 0:
        return theta_cos
    else:
        return 2 * np.pi - theta_cos


def box_rigid_transform(in_box, pose_pre, pose_cur):
    inv_pose_of_last_frame = np.linalg.inv(pose_cur)
    registration_mat = np.matmul(inv_pose_of_last_frame, pose_pre)
    box = copy.deepcopy(in_box)
    angle = get_registration_angle(registration_mat)
    box[0:3] = points_rigid_transform(np.array([box[0:3]]), registration_mat)[0, 0:3]
    box[6] += angle
    return box


def track_prototypes(outline_infos, refiner_cfg):
    """l.496-642: the track tables by outline_ids -> (static, dynamic). static[key][id] is the best-scoring entry of a track whose
    global positions spread less than StaticThresh; dynamic[key][id][frame] the other tracks' boxes with the best entry's size and
    the heading of the track's motion."""
    static_thresh = _get(refiner_cfg, "StaticThresh")
    pos_proto = {k: {} for k in ('pose', 'box', 'proto_id', 'cls', 'score', 'global_position')}
    for i, info in enumerate(outline_infos):
        pose = info['pose']
        for box_i, this_box in enumerate(info['outline_box']):
            ob_id = info['outline_ids'][box_i]
            global_position = points_rigid_transform(np.array([this_box[0:3]]), pose)[:, 0:3]
            for key, val in (('proto_id', info['outline_proto_id'][box_i]), ('pose', pose), ('box', this_box),
                             ('cls', info['outline_cls'][box_i]), ('score', info['outline_score'][box_i]),
                             ('global_position', global_position[0])):
                pos_proto[key].setdefault(ob_id, {})[i] = val
    new_pos_proto_static = {k: {} for k in ('pose', 'box', 'cls', 'proto_id', 'score')}
    new_pos_proto_dynamic = {k: {} for k in ('box', 'cls', 'proto_id', 'score')}
    for ob_id in pos_proto['box'].keys():
        all_score = np.array(list(pos_proto['score'][ob_id].values()))
        all_box = np.array(list(pos_proto['box'][ob_id].values()))
        all_cls = np.array(list(pos_proto['cls'][ob_id].values()))
        all_proto_id = np.array(list(pos_proto['proto_id'][ob_id].values()))
        all_pose = np.array(list(pos_proto['pose'][ob_id].values()))
        all_position = np.array(list(pos_proto['global_position'][ob_id].values()))
        mean_position = np.mean(all_position[:, 0:2], 0)
        dis = np.linalg.norm(all_position[:, 0:2] - mean_position, axis=1)
        std = np.std(dis)
        argmax_score = np.argmax(all_score)
        best_box, best_cls, best_score = all_box[argmax_score], all_cls[argmax_score], all_score[argmax_score]
        best_proto_id = all_proto_id[argmax_score]
        if std < static_thresh:
            new_pos_proto_static['pose'][ob_id] = all_pose[argmax_score]
            new_pos_proto_static['box'][ob_id] = best_box
            new_pos_proto_static['cls'][ob_id] = best_cls
            new_pos_proto_static['score'][ob_id] = best_score
            new_pos_proto_static['proto_id'][ob_id] = best_proto_id
            continue
        for k in new_pos_proto_dynamic:
            new_pos_proto_dynamic[k][ob_id] = {}
        positions = pos_proto['global_position'][ob_id]
        win_size = 10
        for frame_id in pos_proto['box'][ob_id].keys():
            this_box = copy.deepcopy(pos_proto['box'][ob_id][frame_id])
            this_box[3:6] = best_box[3:6]
            new_pos_proto_dynamic['score'][ob_id][frame_id] = best_score
            new_pos_proto_dynamic['box'][ob_id][frame_id] = this_box
            new_pos_proto_dynamic['cls'][ob_id][frame_id] = best_cls
            new_pos_proto_dynamic['proto_id'][ob_id][frame_id] = best_proto_id
            position_left = np.array([positions[k] for k in range(frame_id - win_size + 1, frame_id + 1) if k in positions])
            position_right = np.array([positions[k] for k in range(frame_id, frame_id + win_size) if k in positions])
            angle_vec = np.mean(position_right[:, 0:2], 0) - np.mean(position_left[:, 0:2], 0)
            if np.linalg.norm(angle_vec) > 1:
                global_angle = angle_from_vector(angle_vec[0], angle_vec[1])
                angle_off_from_pose = get_registration_angle(np.linalg.inv(pos_proto['pose'][ob_id][frame_id]))
                this_box[6] = global_angle + angle_off_from_pose
    return new_pos_proto_static, new_pos_proto_dynamic


def refine_box_pos(outline_infos, refiner_cfg):
    """The body of C_PROTO.refine_box_pos (l.496-670) over loaded _resize infos (updated in place and returned). The static
    tracks are written back; the dynamic ones are computed and, as in the reference, left as they are (l.644-670)."""
    score_thresh = _get(refiner_cfg, "BasicProtoScoreThresh")
    new_pos_proto_static, _ = track_prototypes(outline_infos, refiner_cfg)
    for i, info in enumerate(outline_infos):
        for box_i in range(len(info['outline_box'])):
            ob_id = info['outline_ids'][box_i]
            if ob_id not in new_pos_proto_static['box']:
                continue
            propo_cls = new_pos_proto_static['cls'][ob_id]
            proto_score = new_pos_proto_static['score'][ob_id]
            new_box = box_rigid_transform(new_pos_proto_static['box'][ob_id], new_pos_proto_static['pose'][ob_id], info['pose'])
            info['outline_box'][box_i] = new_box[:]
            info['outline_cls'][box_i] = propo_cls
            if propo_cls in score_thresh:
                if proto_score > score_thresh[propo_cls]:
                    info['outline_score'][box_i] = proto_score
            info['outline_proto_id'][box_i] = new_pos_proto_static['proto_id'][ob_id]
    return outline_infos


class C_PROTO(cproto.C_PROTO):
    """c_proto_refine.py:46-683, the whole refiner: the first two stages are cproto.C_PROTO's, refine_box_size writes
    <seq>_outline_<LabelRefiner>_resize.pkl and refine_box_pos <seq>_outline_<LabelRefiner>.pkl, both cached."""

    @property
    def gpu(self):
        if self._gpu is None:
            self._gpu = RefineGPU(self.dataset_cfg, self.device, self.sub_batch)
        return self._gpu

    def _refined_path(self, suffix):
        name = str(_get(self.dataset_cfg, "LabelRefiner"))
        return os.path.join(self.root_path, self.seq_name, self.seq_name + '_outline_' + name + suffix + '.pkl')

    def resize_frames(self, frames, infos, table):
        """l.374-471 for the frames (a list of [N, 3] arrays) that go with infos (updated in place)."""
        css = self.css_estimator
        orien_thresh = _get(_get(self.dataset_cfg, "RefinerConfig"), "OrienThresh")
        seq_id = int(self.seq_name[8:16])
        frames = [np.asarray(f) for f in frames]
        gpu = self.gpu
        if getattr(gpu, "table", None) is not table:
            gpu.set_prototypes(table)
        for i in range(len(frames)):
            infos[i]['outline_proto_id'] = np.ones_like(infos[i]['outline_ids'], dtype=np.longlong) * (-1)
        for c0, c1 in dtype_runs(frames, self.chunk):
            boxes, seg_frame, seg_cls, basic, where = [], [], [], [], []
            for i in range(c0, c1):
                for b in range(len(infos[i]['outline_box'])):
                    name = infos[i]['outline_cls'][b]
                    if name not in table.basic:
                        continue
                    proto_id = int(str(seq_id) + str(infos[i]['outline_ids'][b]))
                    boxes.append(np.array(infos[i]['outline_box'][b], np.float64))
                    seg_frame.append(i - c0)
                    seg_cls.append(CLASSES.index(name))
                    basic.append(table.basic_whl(name, proto_id))
                    where.append((i, b, proto_id))
            res = gpu.run(frames[c0:c1], np.array(boxes).reshape(-1, 7), seg_frame, seg_cls=seg_cls,
                          basic_whl=np.array(basic).reshape(-1, 3))
            for s, (i, b, proto_id) in enumerate(where):
                name = infos[i]['outline_cls'][b]
                new_box = np.array(res["new_box"][s])
                infos[i]['outline_proto_id'][b] = table.proto_id(seg_cls[s], int(res["fit_index"][s]), proto_id)
                if res["best_label"][s] >= 0:
                    css_score = css.from_occ(res["occ"][s], new_box, name)
                    infos[i]['outline_score'][b] = css_score
                    if name == 'Vehicle':
                        new_box = np.array(res["box_orient_drift" if css_score > orien_thresh else "box_drift"][s])
                infos[i]['outline_box'][b] = new_box

    def refine_box_size(self):
        output_info_path = self._refined_path('_resize')
        if os.path.exists(output_info_path):
            with open(output_info_path, 'rb') as f:
                return pkl.load(f)
        with open(self._path('_CSS_proto'), 'rb') as f:
            proto_set = pkl.load(f)
        with open(self._path('_CSS'), 'rb') as f:
            outline_infos = pkl.load(f)
        table = PrototypeTable(proto_set, self.css_estimator.predifined_size)
        for idx, frames in self.frame_chunks(len(outline_infos)):
            self.resize_frames(frames, outline_infos[idx[0]:idx[0] + len(frames)], table)
        with open(output_info_path, 'wb') as f:
            pkl.dump(outline_infos, f)
        return outline_infos

    def refine_box_pos(self):
        output_info_path = self._refined_path('')
        if os.path.exists(output_info_path):
            with open(output_info_path, 'rb') as f:
                return pkl.load(f)
        with open(self._refined_path('_resize'), 'rb') as f:
            outline_infos = pkl.load(f)
        outline_infos = refine_box_pos(outline_infos, _get(self.dataset_cfg, "RefinerConfig"))
        with open(output_info_path, 'wb') as f:
            pkl.dump(outline_infos, f)
        return outline_infos

    def __call__(self):
        self.compute_css_score_and_raw_proto()
        self.construct_prototypes()
        self.refine_box_size()
        return self.refine_box_pos()


def create_refined(seq_names, root_path, dataset_cfg, device=None, chunk=16):
    """Single-process sequence driver (forked workers must not each open the GPU): every sequence's four stages through one
    GPU context. Returns the final infos per sequence."""
    return run_sequences(lambda s: C_PROTO(s, root_path, dataset_cfg, device, chunk), seq_names, lambda c: c())
