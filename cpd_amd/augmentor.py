"""Training-time augmentor and gt-sampling object database on the device.

  random_flip_along_x / _y, global_rotation, global_scaling, random_flip_with_param
                              cpd/datasets/augmentor/augmentor_utils.py:8-105
  DataAugmentor               cpd/datasets/augmentor/data_augmentor.py (num_frames == 1, what dataset.py:53-56 constructs)
  DataBaseSampler             cpd/datasets/augmentor/database_sampler.py:12-144, 359-465
  TestAugmentor               cpd/datasets/augmentor/test_augmentor.py
  create_track_groundtruth_database
                              cpd/datasets/waymo_unsupervised/waymo_unsupervised_dataset.py:653-754
  mask_boxes_outside_range_numpy, prepare_train_points
                              cpd/utils/box_utils.py:55-71; dataset.py:166-173 + data_processor.py:77-126

`points` is a device tensor everywhere; box tables (a few dozen rows), names and the database bookkeeping stay on the host and
are the reference's own numpy / torch-CPU calls, restated. Every function draws from np.random exactly what the reference
draws, in the same order. The point side of a whole DataAugmentor.forward -- paste the sampled objects, remove the scene points
inside the sampled boxes, flip, rotate, scale, range mask -- is ONE cpd_augment_scene call (csrc/augment.hip); the database
writer's point work is cpd_points_in_boxes + cpd_group_points_by_box. There is no host fallback.

Rotated coordinates are not bit-equal to the reference's: torch's CPU float32 matmul fuses x c + y (-s) as fma(y, -s, fl(x c))
for all but tiny N and not for some rows of tiny N; the kernel always uses the fused chain (one float32 ulp of difference at
most). The paste offset and the database centring are float64 operations rounded once (a float32 array and a float64 array);
the scaling is a float32 product by the factor rounded to float32 (np.random.uniform and a yaml number are Python floats, which
numpy multiplies into a float32 array in float32): both are bit-exact against the reference.
"""
import ctypes
import pathlib
import pickle
from functools import partial

import numpy as np
import torch

from . import ops as _ops
from . import prefilter
from ._lib import check, farr, lib, ptr, stream

FLIP_X, FLIP_Y, ROT, SCALE = 0, 1, 2, 3
MAX_OPS = 8


def _get(cfg, key, default=None):
    """cfg.key or cfg[key] (yaml dict, namespace or easydict), `default` when absent."""
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


# ---- host restatements used on box tables ---------------------------------------------------------------------------------
def check_numpy_to_torch(x):
    if isinstance(x, np.ndarray):
        return torch.from_numpy(x).float(), True
    return x, False


def limit_period(val, offset=0.5, period=np.pi):
    val, is_numpy = check_numpy_to_torch(val)
    ans = val - torch.floor(val / period + offset) * period
    return ans.numpy() if is_numpy else ans


def rotate_points_along_z(points, angle):
    """common_utils.py:35-57 on the host (torch CPU float32), for box tables."""
    points, is_numpy = check_numpy_to_torch(points)
    angle, _ = check_numpy_to_torch(angle)
    cosa, sina = torch.cos(angle), torch.sin(angle)
    zeros, ones = angle.new_zeros(points.shape[0]), angle.new_ones(points.shape[0])
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).float()
    out = torch.cat((torch.matmul(points[:, :, 0:3], rot), points[:, :, 3:]), dim=-1)
    return out.numpy() if is_numpy else out


def rotation_cos_sin(angle):
    """The float32 cos / sin rotate_points_along_z gets from torch for a Python / numpy angle."""
    a = torch.from_numpy(np.array([angle])).float()
    return float(torch.cos(a)[0]), float(torch.sin(a)[0])


def boxes_to_corners_3d(boxes3d):
    boxes3d, is_numpy = check_numpy_to_torch(boxes3d)
    template = boxes3d.new_tensor(([1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1],
                                   [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1])) / 2
    corners3d = boxes3d[:, None, 3:6].repeat(1, 8, 1) * template[None, :, :]
    corners3d = rotate_points_along_z(corners3d.view(-1, 8, 3), boxes3d[:, 6]).view(-1, 8, 3)
    corners3d += boxes3d[:, None, 0:3]
    return corners3d.numpy() if is_numpy else corners3d


def mask_boxes_outside_range_numpy(boxes, limit_range, min_num_corners=1):
    """box_utils.py:55-71 (host)."""
    if boxes.shape[1] > 7:
        boxes = boxes[:, 0:7]
    corners = boxes_to_corners_3d(boxes)
    mask = ((corners >= limit_range[0:3]) & (corners <= limit_range[3:6])).all(axis=2)
    return mask.sum(axis=1) >= min_num_corners


def enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    """box_utils.py:136-149: float32 boxes with the sizes grown (host torch)."""
    boxes3d, _ = check_numpy_to_torch(boxes3d)
    large = boxes3d.clone()
    large[:, 3:6] += boxes3d.new_tensor(extra_width)[None, :]
    return large


# ---- the kernel call ------------------------------------------------------------------------------------------------------
def augment_scene(scene, ops=(), limit_range=None, obj_base=None, obj_start=None, obj_count=None, obj_centre=None, boxes=None):
    """cpd_augment_scene: scene [n, c] f32 device; ops = [(kind, p0, p1), ...]; obj_base [rows, c_obj] f32 device with host
    obj_start / obj_count / obj_centre [k_obj, 3] (float64); boxes [k, 7] (host or device) = the boxes whose scene points are
    removed. Returns the kept rows [n_out, c] (one host read of the count)."""
    scene = scene.contiguous()
    assert scene.dtype == torch.float32 and scene.dim() == 2
    dev = scene.device
    n, c = scene.shape
    k_obj = 0 if obj_start is None else len(obj_start)
    start = np.ascontiguousarray(obj_start if k_obj else [], np.int64)
    count = np.ascontiguousarray(obj_count if k_obj else [], np.int32)
    centre = np.ascontiguousarray(np.asarray(obj_centre if k_obj else [], np.float64).reshape(-1, 3))
    assert len(count) == k_obj and len(centre) == k_obj
    m = int(count.astype(np.int64).sum())
    if obj_base is not None:
        obj_base = obj_base.contiguous()
        assert obj_base.dtype == torch.float32 and obj_base.device == dev
    rows, c_obj = (obj_base.shape if obj_base is not None else (0, c))
    if boxes is None:
        bx, k = None, 0
    else:
        bx = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 7).to(dev).contiguous()
        k = bx.shape[0]
    kind = np.ascontiguousarray([o[0] for o in ops], np.int32)
    param = np.ascontiguousarray([[o[1], o[2]] for o in ops], np.float64).reshape(-1, 2)
    if n + m >= 2 ** 31 or k > 512 or k_obj > 512 or len(ops) > MAX_OPS:
        ws_bytes = 256               # the library reports the limit
    else:
        ws_bytes = lib().cpd_augment_scene_workspace_bytes(n, m, k_obj)
    ws = torch.empty((max(int(ws_bytes), 256),), dtype=torch.uint8, device=dev)
    out = torch.empty((max(n + m, 1) if n + m < 2 ** 31 else 1, c), dtype=torch.float32, device=dev)
    n_out = torch.zeros((1,), dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    check(lib().cpd_augment_scene(ptr(scene), n, c, ptr(obj_base), int(rows), int(c_obj), vp(start.ctypes.data), vp(count.ctypes.data),
                                  vp(centre.ctypes.data), k_obj, ptr(bx), k, vp(kind.ctypes.data), vp(param.ctypes.data), len(ops),
                                  farr(limit_range) if limit_range is not None else None, ptr(out), ptr(n_out), ptr(ws), ws.numel(),
                                  stream()), "cpd_augment_scene")
    return out[:int(n_out.item())]


def group_points_by_box(points, box_idx, centres):
    """cpd_group_points_by_box: points [n, c] f32 device, box_idx [n] int32 device (-1 = background), centres [k, 3] host
    float64 -> (rows [n, c] device, grouped by box and centred; offsets [k + 1] device int32)."""
    points = points.contiguous()
    box_idx = box_idx.contiguous()
    assert points.dtype == torch.float32 and box_idx.dtype == torch.int32 and box_idx.numel() == points.shape[0]
    n, c = points.shape
    centre = np.ascontiguousarray(np.asarray(centres, np.float64).reshape(-1, 3))
    k = centre.shape[0]
    ws_bytes = lib().cpd_group_points_by_box_workspace_bytes(n, k) if k <= 1024 else 256
    ws = torch.empty((max(int(ws_bytes), 256),), dtype=torch.uint8, device=points.device)
    out = torch.empty((max(n, 1), c), dtype=torch.float32, device=points.device)
    offsets = torch.zeros((k + 1,), dtype=torch.int32, device=points.device)
    check(lib().cpd_group_points_by_box(ptr(points), n, c, ptr(box_idx), k, ctypes.c_void_p(centre.ctypes.data), ptr(out),
                                        ptr(offsets), ptr(ws), ws.numel(), stream()), "cpd_group_points_by_box")
    return out[:n], offsets


class PointOps:
    """The points of a frame with the work still to do on them: DataAugmentor.forward hands this through its queue instead of
    the tensor, every step appends its op, and `run` makes the one kernel call."""

    def __init__(self, points):
        self.points = points
        self.ops = []
        self.paste = None            # dict(obj_base, obj_start, obj_count, obj_centre, boxes)

    @property
    def shape(self):
        return self.points.shape

    def add(self, kind, p0=0.0, p1=0.0):
        if len(self.ops) == MAX_OPS:
            self.run()
        self.ops.append((kind, float(p0), float(p1)))

    def set_paste(self, **paste):
        if self.ops or self.paste is not None:          # pasted objects must not see the ops collected before them
            self.run()
        self.paste = paste

    def run(self, limit_range=None):
        self.points = augment_scene(self.points, self.ops, limit_range, **(self.paste or {}))
        self.ops, self.paste = [], None
        return self.points


def _point_op(points, kind, p0=0.0, p1=0.0):
    if isinstance(points, PointOps):
        points.add(kind, p0, p1)
        return points
    return augment_scene(points, [(kind, float(p0), float(p1))])


# ---- augmentor_utils.py:8-105 ---------------------------------------------------------------------------------------------
def random_flip_along_x(gt_boxes, points):
    enable = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
    if enable:
        gt_boxes[:, 1] = -gt_boxes[:, 1]
        gt_boxes[:, 6] = -gt_boxes[:, 6]
        points = _point_op(points, FLIP_X)
        if gt_boxes.shape[1] > 7:
            gt_boxes[:, 8] = -gt_boxes[:, 8]
    return gt_boxes, points, enable


def random_flip_along_y(gt_boxes, points):
    enable = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
    if enable:
        gt_boxes[:, 0] = -gt_boxes[:, 0]
        gt_boxes[:, 6] = -(gt_boxes[:, 6] + np.pi)
        points = _point_op(points, FLIP_Y)
        if gt_boxes.shape[1] > 7:
            gt_boxes[:, 7] = -gt_boxes[:, 7]
    return gt_boxes, points, enable


def random_flip_with_param(points, enable, ax=1, offset=0):
    """points: a device tensor / PointOps (ax 0 or 1, no offset) or a host box table (any column)."""
    if enable and points is not None:
        if isinstance(points, np.ndarray):
            points[:, ax] = -(points[:, ax] + offset)
        else:
            if ax not in (0, 1) or offset != 0:
                raise NotImplementedError("random_flip_with_param on device points flips column 0 or 1 without offset")
            points = _point_op(points, FLIP_X if ax == 1 else FLIP_Y)
    return points


def global_rotation(gt_boxes, points, rot_range):
    noise_rotation = np.random.uniform(rot_range[0], rot_range[1])
    cs, sn = rotation_cos_sin(noise_rotation)
    points = _point_op(points, ROT, cs, sn)
    gt_boxes[:, 0:3] = rotate_points_along_z(gt_boxes[np.newaxis, :, 0:3], np.array([noise_rotation]))[0]
    gt_boxes[:, 6] += noise_rotation
    if gt_boxes.shape[1] > 7:
        gt_boxes[:, 7:9] = rotate_points_along_z(
            np.hstack((gt_boxes[:, 7:9], np.zeros((gt_boxes.shape[0], 1))))[np.newaxis, :, :], np.array([noise_rotation]))[0][:, 0:2]
    return gt_boxes, points, noise_rotation


def global_scaling(gt_boxes, points, scale_range):
    if scale_range[1] - scale_range[0] < 1e-3:
        # the reference returns a 2-tuple here and its caller fails to unpack it
        raise ValueError("global_scaling: WORLD_SCALE_RANGE narrower than 1e-3")
    noise_scale = np.random.uniform(scale_range[0], scale_range[1])
    points = _point_op(points, SCALE, noise_scale)
    gt_boxes[:, :6] *= noise_scale
    return gt_boxes, points, noise_scale


# ---- database_sampler.py --------------------------------------------------------------------------------------------------
class DataBaseSampler(object):
    """DataBaseSampler of database_sampler.py (single-frame form). `resident=False` reads the sampled objects' .bin files per
    call, as the reference does, and uploads them packed; `resident=True` packs every object that survives PREPARE into one
    device buffer at construction (4 * NUM_POINT_FEATURES bytes per database point) and a call passes only row starts and
    counts. Both give identical outputs. A class whose filtered database is empty raises ValueError here (the reference spins
    forever in sample_with_fixed_number)."""

    def __init__(self, root_path, sampler_cfg, class_names, num_frames, logger=None, dataset_cfg=None, device=None, resident=False):
        if num_frames != 1:
            raise NotImplementedError("DataBaseSampler: the multi-frame sampler (add_sampled_boxes_to_scene_multi) is not ported")
        for key, why in (("USE_ROAD_PLANE", "road planes are KITTI-only"), ("USE_VAN", "the Van alias is KITTI-only"),
                         ("DATABASE_WITH_FAKELIDAR", "fake-lidar databases are KITTI-only")):
            if _get(sampler_cfg, key, False):
                raise NotImplementedError("DataBaseSampler: %s is not supported (%s)" % (key, why))
        self.root_path = pathlib.Path(root_path)
        self.class_names = class_names
        self.sampler_cfg = sampler_cfg
        self.dataset_cfg = dataset_cfg
        self.logger = logger
        self.num_frames = num_frames
        self.device = torch.device(device if device is not None else "cuda")
        self.resident = bool(resident)
        self.num_point_features = int(_get(sampler_cfg, "NUM_POINT_FEATURES"))
        self.db_infos = {name: [] for name in class_names}
        for db_info_path in _get(sampler_cfg, "DB_INFO_PATH"):
            with open(str(self.root_path.resolve() / db_info_path), "rb") as f:
                infos = pickle.load(f)
            for cls in class_names:
                if cls in infos.keys():
                    self.db_infos[cls].extend(infos[cls])
        for func_name, val in dict(_get(sampler_cfg, "PREPARE")).items():
            self.db_infos = getattr(self, func_name)(self.db_infos, val)
        self.sample_groups = {}
        self.sample_class_num = {}
        self.limit_whole_scene = _get(sampler_cfg, "LIMIT_WHOLE_SCENE", False)
        for x in _get(sampler_cfg, "SAMPLE_GROUPS"):
            class_name, sample_num = x.split(":")
            if class_name not in class_names:
                continue
            if len(self.db_infos[class_name]) == 0:
                raise ValueError("DataBaseSampler: no database object of class %s is left after PREPARE" % class_name)
            self.sample_class_num[class_name] = sample_num
            self.sample_groups[class_name] = {"sample_num": sample_num, "pointer": len(self.db_infos[class_name]),
                                              "indices": np.arange(len(self.db_infos[class_name]))}
        self.last_sampled = []              # the infos pasted by the last call (diagnostics / tests)
        self._rows = {}                     # resident: path -> (first row, rows)
        self._base = None
        if self.resident:
            chunks, at = [], 0
            for name in class_names:
                for info in self.db_infos[name]:
                    if info["path"] in self._rows:
                        continue
                    pts = self._read(info)
                    self._rows[info["path"]] = (at, pts.shape[0])
                    chunks.append(pts)
                    at += pts.shape[0]
            packed = np.concatenate(chunks, 0) if chunks else np.zeros((0, self.num_point_features), np.float32)
            self._base = torch.from_numpy(packed).to(self.device)

    def __getstate__(self):
        d = dict(self.__dict__)
        del d["logger"]
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def _read(self, info):
        return np.fromfile(str(self.root_path / info["path"]), dtype=np.float32).reshape([-1, self.num_point_features])

    def filter_by_difficulty(self, db_infos, removed_difficulty):
        new_db_infos = {}
        for key, dinfos in db_infos.items():
            new_db_infos[key] = [info for info in dinfos if "difficulty" not in info or info["difficulty"] not in removed_difficulty]
            if self.logger is not None:
                self.logger.info("Database filter by difficulty %s: %d => %d" % (key, len(dinfos), len(new_db_infos[key])))
        return new_db_infos

    def filter_by_min_points(self, db_infos, min_gt_points_list):
        for name_num in min_gt_points_list:
            name, min_num = name_num.split(":")
            min_num = int(min_num)
            if min_num > 0 and name in db_infos.keys():
                filtered = [info for info in db_infos[name] if info["num_points_in_gt"] >= min_num]
                if self.logger is not None:
                    self.logger.info("Database filter by min points %s: %d => %d" % (name, len(db_infos[name]), len(filtered)))
                db_infos[name] = filtered
        return db_infos

    def sample_with_fixed_number_previous(self, class_name, sample_group):
        sample_num, pointer, indices = int(sample_group["sample_num"]), sample_group["pointer"], sample_group["indices"]
        if pointer >= len(self.db_infos[class_name]):
            indices = np.random.permutation(len(self.db_infos[class_name]))
            pointer = 0
        sampled_dict = [self.db_infos[class_name][idx] for idx in indices[pointer: pointer + sample_num]]
        method = _get(self.dataset_cfg, "current_label_method")
        new_dict = [s for s in sampled_dict if method in s["labeling_method_dict"]]
        pointer += sample_num
        sample_group["pointer"] = pointer
        sample_group["indices"] = indices
        return new_dict

    def sample_with_fixed_number(self, class_name, sample_group):
        new_dict = []
        sample_num = int(sample_group["sample_num"])
        while len(new_dict) < sample_num:
            new_dict += self.sample_with_fixed_number_previous(class_name, sample_group)
        return new_dict

    def add_sampled_boxes_to_scene(self, data_dict, sampled_gt_boxes, total_valid_sampled_dict):
        gt_boxes_mask = np.array([n in self.class_names for n in data_dict["gt_names"]], dtype=np.bool_)
        gt_boxes = data_dict["gt_boxes"][gt_boxes_mask]
        gt_names = data_dict["gt_names"][gt_boxes_mask]
        if "gt_tracklets" in data_dict:
            data_dict["gt_tracklets"] = data_dict["gt_tracklets"][gt_boxes_mask]
        points = data_dict["points"]
        if self.resident:
            base = self._base
            rows = [self._rows[info["path"]] for info in total_valid_sampled_dict]
            start, count = [r[0] for r in rows], [r[1] for r in rows]
        else:
            objs = [self._read(info) for info in total_valid_sampled_dict]
            count = [o.shape[0] for o in objs]
            start = np.concatenate([[0], np.cumsum(count)[:-1]]).tolist()
            dev = points.points.device if isinstance(points, PointOps) else points.device
            base = torch.from_numpy(np.concatenate(objs, axis=0)).to(dev)
        centre = np.stack([np.asarray(info["box3d_lidar"][:3], np.float64) for info in total_valid_sampled_dict])
        sampled_gt_names = np.array([x["name"] for x in total_valid_sampled_dict])
        large = enlarge_box3d(sampled_gt_boxes[:, 0:7], extra_width=_get(self.sampler_cfg, "REMOVE_EXTRA_WIDTH"))
        paste = dict(obj_base=base, obj_start=start, obj_count=count, obj_centre=centre, boxes=large)
        if isinstance(points, PointOps):
            points.set_paste(**paste)
        else:
            points = augment_scene(points, **paste)
        gt_names = np.concatenate([gt_names, sampled_gt_names], axis=0)
        gt_boxes = np.concatenate([gt_boxes, sampled_gt_boxes], axis=0)
        valid_mask = np.ones((len(gt_names),), dtype=np.bool_)
        valid_mask[:len(gt_names) - len(sampled_gt_names)] = 0
        data_dict["valid_noise"] = valid_mask
        data_dict["gt_boxes"] = gt_boxes
        data_dict["gt_names"] = gt_names
        data_dict["points"] = points
        return data_dict

    def __call__(self, data_dict):
        if "road_plane" in data_dict:
            raise NotImplementedError("DataBaseSampler: road planes are not supported")
        gt_boxes = data_dict["gt_boxes"]
        gt_names = data_dict["gt_names"].astype(str)
        existed_boxes = gt_boxes
        total_valid_sampled_dict = []
        for class_name, sample_group in self.sample_groups.items():
            if self.limit_whole_scene:
                num_gt = np.sum(class_name == gt_names)
                sample_group["sample_num"] = str(int(self.sample_class_num[class_name]) - num_gt)
            if int(sample_group["sample_num"]) > 0:
                sampled_dict = self.sample_with_fixed_number(class_name, sample_group)
                sampled_boxes = np.stack([x["box3d_lidar"] for x in sampled_dict], axis=0).astype(np.float32)
                iou1 = _ops.boxes_iou_bev_cpu(torch.from_numpy(np.ascontiguousarray(sampled_boxes[:, 0:7])),
                                              torch.from_numpy(np.ascontiguousarray(existed_boxes[:, 0:7], np.float32))).numpy()
                iou2 = _ops.boxes_iou_bev_cpu(torch.from_numpy(np.ascontiguousarray(sampled_boxes[:, 0:7])),
                                              torch.from_numpy(np.ascontiguousarray(sampled_boxes[:, 0:7]))).numpy()
                iou2[range(sampled_boxes.shape[0]), range(sampled_boxes.shape[0])] = 0
                iou1 = iou1 if iou1.shape[1] > 0 else iou2
                valid_mask = ((iou1.max(axis=1) + iou2.max(axis=1)) == 0).nonzero()[0]
                valid_sampled_dict = [sampled_dict[x] for x in valid_mask]
                valid_sampled_boxes = sampled_boxes[valid_mask]
                existed_boxes = np.concatenate((existed_boxes, valid_sampled_boxes), axis=0)
                total_valid_sampled_dict.extend(valid_sampled_dict)
        sampled_gt_boxes = existed_boxes[gt_boxes.shape[0]:, :]
        self.last_sampled = total_valid_sampled_dict
        if len(total_valid_sampled_dict) > 0:
            data_dict = self.add_sampled_boxes_to_scene(data_dict, sampled_gt_boxes, total_valid_sampled_dict)
        return data_dict


# ---- data_augmentor.py ----------------------------------------------------------------------------------------------------
class DataAugmentor(object):
    """DataAugmentor of data_augmentor.py for num_frames == 1. forward() keeps the reference's keys: `points` (device),
    `gt_boxes` (heading through limit_period(offset=0.5, period=2 pi)), `gt_names`, `valid_noise` when something was pasted,
    `aug_param`; `calib` / `road_plane` are popped.

    `aug_param` is built exactly as the reference builds it: random_world_flip starts the list (or appends int(enable) to an
    existing one), random_world_rotation OVERWRITES it with [rotation], random_world_scaling appends. With the shipped order
    flip -> rotation -> scaling the result is therefore array([rotation, scale]): the flip is lost. Kept as it is.

    The queue only collects the point ops; the points go through ONE cpd_augment_scene call at the end of forward, and
    `limit_range` does mask_points_by_range in that same call."""

    _UNSUPPORTED = {
        "da_sampling": "DADataBaseSampler is out of scope",
        "random_local_flip": "local augmentations are out of scope",
        "random_local_noise": "noise_per_object is out of scope",
        "random_local_pyramid_aug": "pyramid augmentations are out of scope",
        "random_world_trans": "random_patch_shift reorders the cloud on the host; not ported",
    }

    def __init__(self, root_path, augmentor_configs, class_names, logger=None, num_frames=1, dataset_cfg=None, device=None,
                 resident=False):
        if num_frames != 1:
            raise NotImplementedError("DataAugmentor: only num_frames == 1 (what DatasetTemplate constructs) is supported")
        self.root_path = root_path
        self.class_names = class_names
        self.logger = logger
        self.num_frames = num_frames
        self.dataset_cfg = dataset_cfg
        self.device = device
        self.resident = resident
        self.data_augmentor_queue = []
        is_list = isinstance(augmentor_configs, list)
        aug_config_list = augmentor_configs if is_list else _get(augmentor_configs, "AUG_CONFIG_LIST")
        for cur_cfg in aug_config_list:
            name = _get(cur_cfg, "NAME")
            if not is_list and name in _get(augmentor_configs, "DISABLE_AUG_LIST", []):
                continue
            if name in self._UNSUPPORTED:
                raise NotImplementedError("DataAugmentor: %s: %s" % (name, self._UNSUPPORTED[name]))
            self.data_augmentor_queue.append(getattr(self, name)(config=cur_cfg))

    def __getstate__(self):
        d = dict(self.__dict__)
        del d["logger"]
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def gt_sampling(self, config=None):
        return DataBaseSampler(root_path=self.root_path, sampler_cfg=config, class_names=self.class_names, logger=self.logger,
                               num_frames=self.num_frames, dataset_cfg=self.dataset_cfg, device=self.device, resident=self.resident)

    def random_world_rotation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_rotation, config=config)
        rot_range = _get(config, "WORLD_ROT_ANGLE")
        if not isinstance(rot_range, list):
            rot_range = [-rot_range, rot_range]
        gt_boxes, points, param = global_rotation(data_dict["gt_boxes"], data_dict["points"], rot_range=rot_range)
        data_dict["gt_boxes"] = gt_boxes
        data_dict["points"] = points
        data_dict["aug_param"] = [param]
        return data_dict

    def random_world_flip(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_flip, config=config)
        gt_boxes, points = data_dict["gt_boxes"], data_dict["points"]
        for cur_axis in _get(config, "ALONG_AXIS_LIST"):
            assert cur_axis in ["x", "y"]
            gt_boxes, points, param = (random_flip_along_x if cur_axis == "x" else random_flip_along_y)(gt_boxes, points)
        data_dict["gt_boxes"] = gt_boxes
        data_dict["points"] = points
        if "aug_param" in data_dict:
            data_dict["aug_param"].append(int(param))
        else:
            data_dict["aug_param"] = [param]
        return data_dict

    def random_world_scaling(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_scaling, config=config)
        gt_boxes, points, param = global_scaling(data_dict["gt_boxes"], data_dict["points"], _get(config, "WORLD_SCALE_RANGE"))
        data_dict["gt_boxes"] = gt_boxes
        data_dict["points"] = points
        if "aug_param" in data_dict:
            data_dict["aug_param"].append(param)
        else:
            data_dict["aug_param"] = [param]
        return data_dict

    def forward(self, data_dict, limit_range=None):
        pending = PointOps(data_dict["points"])
        data_dict["points"] = pending
        for cur_augmentor in self.data_augmentor_queue:
            data_dict = cur_augmentor(data_dict=data_dict)
        assert data_dict["points"] is pending
        data_dict["points"] = pending.run(limit_range)
        data_dict["gt_boxes"][:, 6] = limit_period(data_dict["gt_boxes"][:, 6], offset=0.5, period=2 * np.pi)
        if "aug_param" in data_dict:
            data_dict["aug_param"] = np.array(data_dict["aug_param"])
        data_dict.pop("calib", None)
        data_dict.pop("road_plane", None)
        return data_dict


# ---- test_augmentor.py ----------------------------------------------------------------------------------------------------
class TestAugmentor(object):
    """TestAugmentor of test_augmentor.py for num_frames == 1: forward runs the configured world_rotation / world_flip /
    world_scaling in list order on `points` (device, one kernel call); backward runs the reversed queue on the host box tables
    `boxes_lidar` / `boxes_3d` with the reference's sign conventions (rotation by -WORLD_ROT, /= WORLD_SCALE, the pi offset of
    the y flip). A box table met in forward, or points met in backward, get the reference's treatment as well."""
    __test__ = False                     # (not a pytest class)

    def __init__(self, augmentor_configs, class_names, logger=None, num_frames=1):
        if num_frames > 1:
            raise NotImplementedError("TestAugmentor: the multi-frame keys (points-1, ...) are not ported")
        self.class_names = class_names
        self.logger = logger
        self.num_frames = num_frames
        self.data_augmentor_queue = []
        self.test_back_queue = []
        aug_config_list = augmentor_configs if isinstance(augmentor_configs, list) else _get(augmentor_configs, "AUG_CONFIG_LIST")
        for i, cur_cfg in enumerate(aug_config_list):
            self.data_augmentor_queue.append(getattr(self, _get(cur_cfg, "NAME"))(config=cur_cfg))
            back_config = aug_config_list[-(i + 1)]
            self.test_back_queue.append(getattr(self, _get(back_config, "NAME"))(config=back_config))

    def __getstate__(self):
        d = dict(self.__dict__)
        del d["logger"]
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def world_flip(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.world_flip, config=config)
        axis = _get(config, "ALONG_AXIS")
        if axis is None:
            return data_dict
        if "points" in data_dict:
            if axis == "x":
                data_dict["points"] = random_flip_with_param(data_dict["points"], True, ax=1)
            if axis == "y":
                data_dict["points"] = random_flip_with_param(data_dict["points"], True, ax=0)
        for key in ("boxes_lidar", "boxes_3d"):
            if key in data_dict:
                boxes = data_dict[key]
                if axis == "x":
                    boxes = random_flip_with_param(boxes, True, ax=1)
                    boxes = random_flip_with_param(boxes, True, ax=6)
                if axis == "y":
                    boxes = random_flip_with_param(boxes, True, ax=0)
                    boxes = random_flip_with_param(boxes, True, ax=6, offset=np.pi)
                data_dict[key] = boxes
        return data_dict

    def world_rotation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.world_rotation, config=config)
        rot_factor = _get(config, "WORLD_ROT")
        if "points" in data_dict:
            cs, sn = rotation_cos_sin(rot_factor)
            data_dict["points"] = _point_op(data_dict["points"], ROT, cs, sn)
        for key in ("boxes_lidar", "boxes_3d"):
            if key in data_dict:
                boxes = data_dict[key]
                boxes[:, 0:3] = rotate_points_along_z(boxes[np.newaxis, :, 0:3], np.array([-rot_factor]))[0]
                boxes[:, 6] += -rot_factor
                data_dict[key] = boxes
        return data_dict

    def world_scaling(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.world_scaling, config=config)
        scale_factor = _get(config, "WORLD_SCALE")
        if "points" in data_dict:
            data_dict["points"] = _point_op(data_dict["points"], SCALE, scale_factor)
        for key in ("boxes_lidar", "boxes_3d"):
            if key in data_dict:
                boxes = data_dict[key]
                boxes[:, 0:6] /= scale_factor
                data_dict[key] = boxes
        return data_dict

    def _run(self, queue, data_dict):
        pending = None
        if "points" in data_dict:
            pending = PointOps(data_dict["points"])
            data_dict["points"] = pending
        for cur_augmentor in queue:
            data_dict = cur_augmentor(data_dict=data_dict)
        if pending is not None:
            data_dict["points"] = pending.run()
        return data_dict

    def forward(self, data_dict):
        return self._run(self.data_augmentor_queue, data_dict)

    def backward(self, data_dict):
        return self._run(self.test_back_queue, data_dict)


# ---- dataset.py:166-173 + data_processor.py:77-126 ------------------------------------------------------------------------
def prepare_train_points(data_dict, point_cloud_range, remove_outside_boxes, shuffle=True, augmentor=None, min_num_corners=1):
    """What prepare_data's augmentor call and the first two DATA_PROCESSOR steps (mask_points_and_boxes_outside_range,
    shuffle_points) give for `points` and `gt_boxes`: augment and range mask in one kernel call, the box mask when
    REMOVE_OUTSIDE_BOXES, one read-back of the count, then np.random.permutation(count) and prefilter.shuffle_points.
    `augmentor` is the DataAugmentor (None: no augmentation, the eval path). Order: the reference selects the classes and
    appends the class column from `gt_names` (dataset.py:199-211) BETWEEN the augmentor and the data processor, so its box mask
    acts on boxes that already carry their class. Here the box mask comes first; `gt_names` and `valid_noise` are therefore
    masked together with `gt_boxes` and stay row for row with them: do the class selection and append the class column after
    this call, from the returned `gt_names`. `points1`, when present, is range-masked and
    shuffled but NOT augmented: the reference's num_frames=1 augmentor never touches it, and that is what the model was
    trained with. Kept as it is."""
    pcr = np.asarray(point_cloud_range, np.float32)
    if augmentor is not None:
        data_dict = augmentor.forward(data_dict, limit_range=pcr)
    else:
        data_dict["points"] = augment_scene(data_dict["points"], limit_range=pcr)
    extra = [k for k in ("points1",) if k in data_dict]
    for key in extra:
        data_dict[key] = augment_scene(data_dict[key], limit_range=pcr)
    if data_dict.get("gt_boxes", None) is not None and remove_outside_boxes:
        mask = mask_boxes_outside_range_numpy(data_dict["gt_boxes"], pcr, min_num_corners=min_num_corners)
        data_dict["gt_boxes"] = data_dict["gt_boxes"][mask]
        for key in ("gt_names", "valid_noise"):              # kept row for row with gt_boxes (see the docstring)
            if key in data_dict:
                data_dict[key] = data_dict[key][mask]
    if shuffle:
        for key in ["points"] + extra:
            perm = np.random.permutation(data_dict[key].shape[0])
            data_dict[key] = prefilter.shuffle_points(data_dict[key], torch.from_numpy(perm))
    return data_dict


# ---- waymo_unsupervised_dataset.py:653-754 --------------------------------------------------------------------------------
def map_to_real_label(outline_box, outline_ids, outline_cls):
    """map_to_real_label(is_str=True) of waymo_unsupervised_dataset.py:625-651."""
    if len(outline_cls) == 0:
        return np.empty(shape=(0,)), np.empty(shape=(0, 7)), np.empty(shape=(0,)), np.empty(shape=(0,))
    n = len(outline_cls)
    return (np.array([outline_cls[i] for i in range(n)]), np.array([outline_box[i] for i in range(n)]),
            np.array([outline_ids[i] for i in range(n)]), np.array([1] * n))


def create_track_groundtruth_database(infos, data_path, save_path, used_classes, split="train", get_lidar=None, device=None):
    """create_track_groundtruth_database: per class (Vehicle on every 10th info, Pedestrian on every 5th, any other class on
    every info), the points of every pseudo-label box, centred on the box, into
    <save_path>/pcdet_gt_track_database_<split>_cp/<seq>/<sample_idx>/<name>_<id>.bin (float32 rows) and the infos into
    pcdet_waymo_track_dbinfos_<split>_cp.pkl, with the reference's keys. Objects of 5 points or fewer are skipped.
    `get_lidar(sequence_name, sample_idx)` -> [N, C] float32 host array (default: <data_path>/<seq>/%04d.npy). A frame is
    uploaded once and kept for the classes that need it; per (frame, class): one cpd_points_in_boxes over that class's boxes
    (so "first containing box" is per class, as in the reference), one cpd_group_points_by_box, one read-back. Directories are
    created (the reference assumes they exist). Returns the dbinfos dict."""
    dev = torch.device(device if device is not None else "cuda")
    data_path, save_path = pathlib.Path(data_path), pathlib.Path(save_path)
    if get_lidar is None:
        def get_lidar(sequence_name, sample_idx):
            return np.load(str(data_path / sequence_name / ("%04d.npy" % sample_idx)))
    gt_path_name = pathlib.Path("pcdet_gt_track_database_%s_cp" % split)
    database_save_path = save_path / gt_path_name
    db_info_save_path = save_path / ("pcdet_waymo_track_dbinfos_%s_cp.pkl" % split)
    database_save_path.mkdir(parents=True, exist_ok=True)
    all_db_infos = {cls_name: [] for cls_name in used_classes}

    def wanted(cls_name, k):
        return not ((cls_name == "Vehicle" and k % 10 != 0) or (cls_name == "Pedestrian" and k % 5 != 0))

    # the reference walks class by class; here frame by frame (one upload per frame) into per-class lists: the same order
    for k in range(len(infos)):
        classes = [c for c in used_classes if wanted(c, k)]
        if not classes:
            continue
        info = infos[k]
        pc_info = info["point_cloud"]
        sequence_name, sample_idx = pc_info["lidar_sequence"], pc_info["sample_idx"]
        if len(info["outline_cls"]) == 0:
            continue
        names_all, boxes_all, ids_all, dif_all = map_to_real_label(info["outline_box"], info["outline_ids"], info["outline_cls"])
        dev_points = None
        for cls_name in classes:
            mask = (names_all == cls_name)
            names, gt_boxes, difficulty, obj_ids = names_all[mask], boxes_all[mask], dif_all[mask], ids_all[mask]
            num_obj = gt_boxes.shape[0]
            if num_obj == 0:
                continue
            if dev_points is None:
                dev_points = torch.from_numpy(np.ascontiguousarray(get_lidar(sequence_name, sample_idx), np.float32)).to(dev)
            bx = torch.from_numpy(np.ascontiguousarray(gt_boxes[:, 0:7])).float().to(dev)
            box_idx = prefilter.points_in_boxes_gpu(dev_points[:, 0:3].unsqueeze(0), bx.unsqueeze(0))[0]
            rows, offsets = group_points_by_box(dev_points, box_idx, gt_boxes[:, :3])
            offsets = offsets.cpu().numpy()
            rows = rows[:int(offsets[-1])].cpu().numpy()             # (the one read-back: offsets and rows of this class)
            for i in range(num_obj):
                ob_id = obj_ids[i]
                filename = "%s_%s.bin" % (names[i], ob_id)
                filepath = database_save_path / sequence_name / str(sample_idx) / filename
                gt_points = rows[offsets[i]:offsets[i + 1]]
                if gt_points.shape[0] <= 5:
                    continue
                filepath.parent.mkdir(parents=True, exist_ok=True)
                with open(filepath, "wb") as f:
                    gt_points.tofile(f)
                db_path = str(gt_path_name / sequence_name / str(sample_idx) / filename)
                all_db_infos[cls_name].append({
                    "name": cls_name, "path": db_path, "sequence_name": sequence_name, "seq_idx": sequence_name,
                    "image_idx": sample_idx, "sample_idx": sample_idx, "gt_idx": i, "ob_idx": ob_id,
                    "box3d_lidar": gt_boxes[i], "num_points_in_gt": gt_points.shape[0], "pose": info["pose"],
                    "difficulty": difficulty[i], "labeling_method_dict": ["unlabeled"]})
    with open(db_info_save_path, "wb") as f:
        pickle.dump(all_db_infos, f)
    return all_db_infos
