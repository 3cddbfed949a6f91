"""KITTI transfer evaluation of a Waymo-trained detector: Kitti2WaymoDataset without the dataset
(cpd/datasets/kitti/kitti2waymo_dataset.py; tools/cfgs/models/waymo_unsupervised/voxel_rcnn_cproto_center_kitti.yaml).

Two stages of that dataset sit on either side of the detector, and both are one kernel call per batch here (csrc/kitti2waymo.hip):

    calibs = [Calibration(root / "calib" / ("%s.txt" % i)) for i in ids]
    points = fov_points(clouds, calibs, image_shapes)                       # __getitem__ l.414-425: FOV crop, z + 1.55, features 0
    preds = engine.forward(points)
    annos = generate_prediction_dicts({"frame_id": ids, "calib": calibs, "image_shape": image_shapes}, preds, class_names)
    result_str, ret_dict = evaluation(annos, gt_annos, class_names)         # kitti_eval.get_official_eval_result

`evaluate_split` is that loop over a split. `camera_keys` recomputes the camera-frame keys of a fused list (the part of
DetectionsMerger.merge that wbf.merge_frames leaves out), `waymo_prediction_dicts` is the Waymo sibling that produces
wbf.merge_frames' input. `Calibration` and the box conversions are host functions with the names, signatures, dtypes and in-place effects of
cpd/utils/calibration_kitti.py and cpd/utils/box_utils.py:91-105,152-235, written afresh and pinned by the golden;
ground-truth conversion is a handful of boxes per frame and stays on the host.

Number formats are the reference's under numpy >= 2 (a float32 scalar stays float32 against a Python number; numpy 1 promotes
`weight * 0.3` of the centre shift to float64). Deviations, on purpose:
  * the caller's tensors and arrays are NOT written (the reference edits a `.cpu().numpy()` copy of the predictions, and
    DetectionsMerger.merge edits the fused boxes it was handed);
  * the kernels take M = np.dot(V2C.T, R0.T) as float32. A calibration file WITHOUT an R0_rect line makes the reference fall back
    to a hard-coded float64 R0, which turns its M, and with it `location`, into float64; the host methods of `Calibration` keep
    that, the kernels round M to float32 once;
  * `pred_boxes` must have exactly seven columns (ValueError otherwise; the reference would carry extra columns into `boxes_lidar`);
  * the host functions are written on the affine parts of the matrices: their values can differ from the reference's homogeneous
    matrix products in the last float32 digit, their dtypes and in-place effects do not;
  * `camera_keys` computes in float32 whatever the dtype of the `boxes_lidar` it is given (merge_frames hands float32 on).
Both kernels are injectable (`_fov=`, `_export=`: the numpy restatement of tests/ref_kitti2waymo.py has the same signatures), so
the host logic runs on a machine without a GPU.
"""
import copy
import os

import numpy as np
import torch

from . import ops

FRAME_WORDS = ops.K2W_FRAME_WORDS                                  # CPD_K2W_FRAME_WORDS
TILE = ops.K2W_TILE                                                # CPD_K2W_TILE
MODE_PREDICT, MODE_CAMERA = ops.K2W_PREDICT, ops.K2W_CAMERA        # CPD_K2W_PREDICT / CPD_K2W_CAMERA
SENSOR_LIFT = 1.55                                                 # kitti2waymo_dataset.py:419 / 277


# ---- calibration (the surface of cpd/utils/calibration_kitti.py) -------------------------------------------------------------

# R0 of a calib file that has no R0_rect / R_rect line: the reference's constant, float64 (every parsed matrix is float32)
DEFAULT_R0 = np.array([[0.99992624, 0.00965411, -0.0072371],
                       [-0.00968531, 0.99994343, -0.00433077],
                       [0.00719491, 0.00440054, 0.99996366]], np.float64)
# line prefix -> (key of the result, matrix shape); a later line of the same key replaces an earlier one
_CALIB_LINES = (("P2", "P2", (3, 4)), ("P3", "P3", (3, 4)), ("Tr_velo_to_cam", "Tr_velo2cam", (3, 4)), ("Tr_velo_cam", "Tr_velo2cam", (3, 4)),
                ("R0_rect", "R0", (3, 3)), ("R_rect", "R0", (3, 3)))


def get_calib_from_file(filepath):
    """A KITTI calib file -> {'P2', 'P3', 'Tr_velo2cam', 'R0'}: the last 12 (9 for R0) numbers of the P2 / P3 / Tr_velo_to_cam
    (Tr_velo_cam) / R0_rect (R_rect) lines as float32; DEFAULT_R0 (float64) when the file names no R0."""
    found = {"R0": DEFAULT_R0.copy()}
    with open(filepath) as f:
        for line in f:
            for prefix, key, shape in _CALIB_LINES:
                if line.startswith(prefix):
                    found[key] = np.array(line.split()[-shape[0] * shape[1]:], np.float32).reshape(shape)
    missing = [k for k in ("P2", "P3", "Tr_velo2cam") if k not in found]
    if missing:
        raise KeyError("%s: no %s line" % (filepath, " / ".join(missing)))
    return found


class Calibration(object):
    """The reference's Calibration: built from a calib file path or a dict with P2 / R0 / Tr_velo2cam; attributes P2 (3 x 4), R0
    (3 x 3), V2C (3 x 4), cu, cv, fu, fv, tx, ty; host methods lidar_to_rect, rect_to_lidar, rect_to_img, lidar_to_img,
    corners3d_to_img_boxes with the reference's result dtypes (float32 from float32 matrices; a float64 R0 makes lidar_to_rect
    float64). Written on the affine parts of the matrices, so values may differ from the reference's homogeneous products in the
    last float32 digit; the device path is fov_points / generate_prediction_dicts."""

    def __init__(self, calib_file):
        calib = calib_file if isinstance(calib_file, dict) else get_calib_from_file(calib_file)
        self.P2, self.R0, self.V2C = calib["P2"], calib["R0"], calib["Tr_velo2cam"]
        (self.fu, _, self.cu, shift_u), (_, self.fv, self.cv, shift_v) = self.P2[0], self.P2[1]
        self.tx, self.ty = shift_u / (-self.fu), shift_v / (-self.fv)

    def lidar_matrix(self):
        """[x y z 1] -> rectified camera frame, 4 x 3: the product the kernels' frame record carries"""
        return np.dot(self.V2C.T, self.R0.T)

    def lidar_to_rect(self, pts_lidar):
        m = self.lidar_matrix()
        return np.asarray(pts_lidar) @ m[:3] + m[3]

    def rect_to_lidar(self, pts_rect):
        full = np.dot(self.R0, self.V2C)                                 # rect = full[:, :3] lidar + full[:, 3]
        return np.linalg.solve(full[:, :3], (np.asarray(pts_rect) - full[:, 3]).T).T

    def rect_to_img(self, pts_rect):
        """-> (pixel coordinates [n, 2], depth [n]); the pixel is divided by the rectified z, as the reference does"""
        pts_rect = np.asarray(pts_rect)
        hom = pts_rect @ self.P2[:, :3].T + self.P2[:, 3]
        return hom[:, :2] / pts_rect[:, 2:3], hom[:, 2] - self.P2[2, 3]

    def lidar_to_img(self, pts_lidar):
        return self.rect_to_img(self.lidar_to_rect(pts_lidar))

    def corners3d_to_img_boxes(self, corners3d):
        """corners [n, 8, 3] in the rectified frame -> (boxes [n, 4] = x1, y1, x2, y2; corner pixels [n, 8, 2]), float64, each pixel
        divided by its own homogeneous coordinate"""
        hom = np.asarray(corners3d, np.float64) @ self.P2[:, :3].T + self.P2[:, 3]
        pix = hom[..., :2] / hom[..., 2:3]
        return np.concatenate([pix.min(axis=1), pix.max(axis=1)], axis=1), pix


# ---- host box conversions (the surface of cpd/utils/box_utils.py and Kitti2WaymoDataset.get_fov_flag) -----------------------

def get_fov_flag(pts_rect, img_shape, calib):
    """points of the rectified frame that fall inside the (h, w) image and not behind it"""
    pix, depth = calib.rect_to_img(pts_rect)
    height, width = img_shape[0], img_shape[1]
    inside = (pix[:, 0] >= 0) & (pix[:, 0] < width) & (pix[:, 1] >= 0) & (pix[:, 1] < height)
    return inside & (depth >= 0)


def boxes3d_kitti_camera_to_lidar(boxes3d_camera, calib):
    """[n, 7] x, y, z, l, h, w, ry in the rectified frame (bottom centre) -> x, y, z, dx, dy, dz, heading in the lidar frame (centre)"""
    cam = np.asarray(boxes3d_camera)
    centre = calib.rect_to_lidar(cam[:, 0:3])
    centre[:, 2] += cam[:, 4] / 2
    return np.column_stack([centre, cam[:, 3], cam[:, 5], cam[:, 4], -(cam[:, 6] + np.pi / 2)])


def boxes3d_lidar_to_kitti_camera(boxes3d_lidar, calib):
    """The inverse. Like the reference it lowers boxes3d_lidar[:, 2] to the bottom face IN PLACE (generate_prediction_dicts' and
    merge's stored boxes_lidar rely on it)."""
    boxes3d_lidar[:, 2] -= boxes3d_lidar[:, 5] / 2
    centre = calib.lidar_to_rect(boxes3d_lidar[:, 0:3])
    return np.column_stack([centre, boxes3d_lidar[:, 3], boxes3d_lidar[:, 5], boxes3d_lidar[:, 4], -boxes3d_lidar[:, 6] - np.pi / 2])


# corner k of a camera-frame box in units of (l / 2, h, w / 2): 0-3 the bottom face, 4-7 the top (y points down)
_CORNER_X = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float32)
_CORNER_Y = np.array([0, 0, 0, 0, -1, -1, -1, -1], np.float32)
_CORNER_Z = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float32)


def boxes3d_to_corners3d_kitti_camera(boxes3d):
    """[n, 7] camera boxes (y at the bottom face) -> corners [n, 8, 3] float32, turned by ry about the y axis"""
    b = np.asarray(boxes3d)
    along, up, across = b[:, 3:4] / 2 * _CORNER_X, b[:, 4:5] * _CORNER_Y, b[:, 5:6] / 2 * _CORNER_Z
    c, s = np.cos(b[:, 6:7]), np.sin(b[:, 6:7])
    return np.stack([b[:, 0:1] + (along * c + across * s), b[:, 1:2] + up, b[:, 2:3] + (across * c - along * s)], axis=2).astype(np.float32)


def boxes3d_kitti_camera_to_imageboxes(boxes3d, calib, image_shape=None):
    """[n, 7] camera boxes -> [n, 4] x1, y1, x2, y2 round the projected corners, clipped to the (h, w) image when it is given"""
    pix, _ = calib.rect_to_img(boxes3d_to_corners3d_kitti_camera(boxes3d).reshape(-1, 3))
    pix = pix.reshape(-1, 8, 2)
    boxes = np.concatenate([pix.min(axis=1), pix.max(axis=1)], axis=1)
    if image_shape is not None:
        boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, image_shape[1] - 1)
        boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, image_shape[0] - 1)
    return boxes


# ---- the per-frame record of both kernels ---------------------------------------------------------------------------------

def frame_words(calibs, image_shapes):
    """int32 [B, FRAME_WORDS]: M = np.dot(V2C.T, R0.T) (formed as Calibration.lidar_to_rect forms it, then float32), P2 (float32),
    image height and width."""
    out = np.zeros((len(calibs), FRAME_WORDS), np.int32)
    for i, (calib, shape) in enumerate(zip(calibs, image_shapes)):
        m = np.ascontiguousarray(np.dot(calib.V2C.T, calib.R0.T), np.float32)      # (any object with V2C / R0 / P2 will do)
        p = np.ascontiguousarray(calib.P2, np.float32)
        assert m.shape == (4, 3) and p.shape == (3, 4)
        out[i, 0:12] = m.reshape(-1).view(np.int32)
        out[i, 12:24] = p.reshape(-1).view(np.int32)
        out[i, 24], out[i, 25] = int(shape[0]), int(shape[1])
    return out


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=off[1:])
    assert off[-1] < 2 ** 31
    return off.astype(np.int32)


def _upload_tables(start, frames, dev):
    """frame offsets and frame records in one copy -> (start [B + 1], frames [B, FRAME_WORDS]) int32 on the device"""
    both = torch.from_numpy(np.concatenate([start, frames.reshape(-1)])).to(dev)
    return both[:len(start)], both[len(start):].view(-1, FRAME_WORDS)


# ---- the input stage ------------------------------------------------------------------------------------------------------

def fov_device(points, frame_start, frames, z_shift, n_feat_out, device="cuda"):
    """The device form of the `_fov=` hook: packed `points` [n, ld] float32 (a host array, uploaded once, or a device tensor), host
    frame_start int32 [B + 1] and frames int32 [B, FRAME_WORDS]. One cpd_kitti_fov_points call, one read-back of the B counts.
    -> (out [n, n_feat_out] device tensor, counts [B] host array); frame f's kept rows start at row frame_start[f]."""
    if isinstance(points, torch.Tensor):
        pts = points if points.is_cuda else points.to(device)
    else:
        pts = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(device)
    pts = pts.contiguous()
    start, fr = _upload_tables(frame_start, frames, pts.device)
    lens = np.diff(frame_start)
    out, count = ops.kitti_fov_points(pts, start, int(lens.max(initial=0)), fr, z_shift, n_feat_out)
    count = count.cpu().numpy()
    if (count < 0).any():
        raise ValueError("cpd_kitti_fov_points refused a frame (bounds out of range)")
    return out, count


def fov_points(points_list, calibs, image_shapes, z_shift=SENSOR_LIFT, num_features=4, _fov=None):
    """The point stage of Kitti2WaymoDataset.__getitem__ (l.414-425) for a batch of frames: per frame keep the points that project
    into the image (lidar_to_rect, get_fov_flag), in their order, lift z by `z_shift` (a float64 sum rounded once to float32) and
    zero every feature. `points_list`: per frame [n_i, ld >= 3] float32, numpy arrays (packed and uploaded in one copy) or tensors;
    `calibs`: Calibration per frame; `image_shapes`: (h, w) per frame. Returns a list of [kept_i, num_features] float32 device
    tensors (views of one buffer), ready for CenterPointEngine / VoxelRCNNEngine.forward. One launch pair and one read-back of
    the B counts per batch."""
    assert len(points_list) == len(calibs) == len(image_shapes)
    if not points_list:
        return []
    frame_start = _offsets([len(p) for p in points_list])
    frames = frame_words(calibs, image_shapes)
    if all(isinstance(p, torch.Tensor) for p in points_list):
        packed = torch.cat([p.to(torch.float32) for p in points_list], 0)
    else:
        packed = np.concatenate([p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p, np.float32) for p in points_list], 0)
    out, count = (_fov or fov_device)(packed, frame_start, frames, float(z_shift), int(num_features))
    out = out if isinstance(out, torch.Tensor) else torch.from_numpy(out)
    return [out[int(s):int(s) + int(c)] for s, c in zip(frame_start[:-1], count)]


# ---- the output stage -----------------------------------------------------------------------------------------------------

def export_device(boxes, scores, labels, seg_start, frames, mode, device="cuda"):
    """The device form of the `_export=` hook: boxes [n, 7] float32 / scores [n] float32 / labels [n] integer (tensors on the device,
    or host arrays), host seg_start int32 [B + 1] and frames int32 [B, FRAME_WORDS]. One cpd_kitti_export launch, one copy back.
    -> dict of host arrays, frame f's kept rows from row seg_start[f]: boxes_lidar [n, 7], score [n], label [n] int32, camera [n, 7]
    (location, dimensions, rotation_y), alpha [n], bbox [n, 4], count [B]."""
    def dev(x, dtype):
        if x is None:
            return None
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=t.device if t.is_cuda else device, dtype=dtype).contiguous()

    b = dev(boxes, torch.float32).view(-1, 7)
    start, fr = _upload_tables(seg_start, frames, b.device)
    got = ops.kitti_export(b, dev(scores, torch.float32), dev(labels, torch.int32), start, fr, mode)
    host = got["buffer"].cpu().numpy()
    n, batch = b.shape[0], len(seg_start) - 1
    f32 = lambda a, shape: a.view(np.float32).reshape(shape)
    out = {"boxes_lidar": f32(host[:7 * n], (n, 7)), "score": f32(host[7 * n:8 * n], (n,)), "label": host[8 * n:9 * n],
           "camera": f32(host[9 * n:16 * n], (n, 7)), "alpha": f32(host[16 * n:17 * n], (n,)), "bbox": f32(host[17 * n:21 * n], (n, 4)),
           "count": host[21 * n:21 * n + batch]}
    if (out["count"] < 0).any():
        raise ValueError("cpd_kitti_export refused a frame (bounds out of range)")
    return out


def _cat_predictions(pred_dicts):
    boxes = [d["pred_boxes"] for d in pred_dicts]
    if any(b.dim() != 2 or b.shape[1] != 7 for b in boxes):
        raise ValueError("generate_prediction_dicts: pred_boxes must be [n, 7] (x, y, z, l, w, h, heading)")
    seg_start = _offsets([len(b) for b in boxes])
    return (torch.cat(boxes, 0).to(torch.float32).contiguous(), torch.cat([d["pred_scores"].reshape(-1) for d in pred_dicts]).to(torch.float32),
            torch.cat([d["pred_labels"].reshape(-1) for d in pred_dicts]).to(torch.int32), seg_start)


def _run_export(export, boxes, scores, labels, seg_start, frames, mode):
    if export is None:
        return export_device(boxes, scores, labels, seg_start, frames, mode)
    host = lambda x: None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))
    return export(host(boxes), host(scores), host(labels), seg_start, frames, mode)


# keys of a KITTI annotation in the reference's order, with the shape each row has
_ANNO_ROWS = (('name', ()), ('truncated', ()), ('occluded', ()), ('alpha', ()), ('bbox', (4,)), ('dimensions', (3,)), ('location', (3,)),
              ('rotation_y', ()), ('score', ()), ('boxes_lidar', (7,)))


def get_template_prediction(num_samples):
    """the annotation of a frame before it is filled: float64 zeros under every key (what a frame without a box keeps)"""
    return {key: np.zeros((num_samples,) + row) for key, row in _ANNO_ROWS}


def _camera_fields(d, got, a, k):
    cam = got["camera"][a:a + k]
    d['alpha'], d['bbox'] = got["alpha"][a:a + k].copy(), got["bbox"][a:a + k].copy()
    d['dimensions'], d['location'], d['rotation_y'] = cam[:, 3:6].copy(), cam[:, 0:3].copy(), cam[:, 6].copy()


def write_kitti_txt(path, anno):
    """One KITTI result line per detection: name, truncation and occlusion as -1, then alpha, the image box, the dimensions as
    height width length (they are stored l, h, w), the location, rotation_y and the score, each with four decimals."""
    order = [1, 2, 0]
    with open(path, 'w') as f:
        for i, name in enumerate(anno['name']):
            numbers = [anno['alpha'][i], *anno['bbox'][i], *anno['dimensions'][i][order], *anno['location'][i], anno['rotation_y'][i],
                       anno['score'][i]]
            f.write("%s -1 -1 %s\n" % (name, " ".join("%.4f" % v for v in numbers)))


def generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None, _export=None):
    """Kitti2WaymoDataset.generate_prediction_dicts (l.246-380), same annos list: per frame the keys name, truncated, occluded, alpha,
    bbox, dimensions, location, rotation_y, score, boxes_lidar (float32 where the reference's are, `name` a string array, truncated /
    occluded float64 zeros) and frame_id; a frame left without a box is the template of float64 zeros. batch_dict: frame_id, calib
    (Calibration), image_shape per frame; pred_dicts: pred_boxes [n, 7] / pred_scores / pred_labels (1-based) tensors per frame,
    not written. With `output_path` each frame's `%s.txt` is written. One launch and one copy back per batch."""
    if not pred_dicts:
        return []
    boxes, scores, labels, seg_start = _cat_predictions(pred_dicts)
    frames = frame_words(batch_dict['calib'][:len(pred_dicts)], batch_dict['image_shape'][:len(pred_dicts)])
    got = _run_export(_export, boxes, scores, labels, seg_start, frames, MODE_PREDICT)
    annos = []
    for index in range(len(pred_dicts)):
        a, k = int(seg_start[index]), int(got["count"][index])
        d = get_template_prediction(k)
        if k:
            d['name'] = np.array(class_names)[got["label"][a:a + k].astype(np.int64) - 1]
            _camera_fields(d, got, a, k)
            d['score'] = got["score"][a:a + k].copy()
            d['boxes_lidar'] = got["boxes_lidar"][a:a + k].copy()
        frame_id = batch_dict['frame_id'][index]
        d['frame_id'] = frame_id
        annos.append(d)
        if output_path is not None:
            write_kitti_txt(os.path.join(str(output_path), '%s.txt' % frame_id), d)
    return annos


def camera_keys(infos, calibs, image_shapes, _export=None):
    """The camera block of DetectionsMerger.merge (merge_detections.py:243-255) for a fused list, e.g. wbf.merge_frames' result:
    per frame `boxes_lidar` gets z += h / 2, goes through boxes3d_lidar_to_kitti_camera (whose in-place z -= h / 2 the stored
    boxes_lidar keeps) and boxes3d_kitti_camera_to_imageboxes; alpha, bbox, dimensions, location, rotation_y are replaced. Returns a
    deep copy of `infos`; the argument is not written. float32 throughout. One launch and one copy back for the whole list."""
    out = copy.deepcopy(infos)
    if not out:
        return out
    boxes = []
    for info in out:
        b = np.array(info['boxes_lidar'], np.float32).reshape(-1, 7)
        b[:, 2] += b[:, 5] / 2
        boxes.append(b)
    seg_start = _offsets([len(b) for b in boxes])
    got = _run_export(_export, np.concatenate(boxes, 0), None, None, seg_start, frame_words(calibs, image_shapes), MODE_CAMERA)
    for index, info in enumerate(out):
        a, k = int(seg_start[index]), int(got["count"][index])
        assert k == len(boxes[index])
        _camera_fields(info, got, a, k)
        info['boxes_lidar'] = got["boxes_lidar"][a:a + k].copy()
    return out


def waymo_prediction_dicts(batch_dict, pred_dicts, class_names, label_offset=0.0, test_augmentor=None):
    """WaymoUnsupervisedDataset.generate_prediction_dicts (waymo_unsupervised_dataset.py:504-558): per frame name / score /
    boxes_lidar (+ frame_id, seq_id), the z of label-1 boxes raised by `label_offset` (dataset_cfg LABEL_OFFSET; a float32 sum on the
    device), then `test_augmentor.backward` when a TestAugmentor is given: the producer of wbf.merge_frames' per-view lists. A frame
    without a box is the template of float64 zeros. The caller's tensors are not written."""
    annos = []
    for index, box_dict in enumerate(pred_dicts):
        scores, boxes, labels = box_dict['pred_scores'], box_dict['pred_boxes'], box_dict['pred_labels']
        n = int(scores.shape[0])
        d = {'name': np.zeros(n), 'score': np.zeros(n), 'boxes_lidar': np.zeros([n, 7])}
        if n:
            mask_car = labels == 1
            boxes = boxes.clone()
            boxes[:, 2] = torch.where(mask_car, boxes[:, 2] + label_offset, boxes[:, 2])
            d['name'] = np.array(class_names)[labels.cpu().numpy() - 1]
            d['score'] = scores.cpu().numpy()
            d['boxes_lidar'] = boxes.cpu().numpy()
        if test_augmentor is not None:
            d = test_augmentor.backward(d)
        d['frame_id'] = batch_dict['frame_id'][index]
        d['seq_id'] = batch_dict['seq_id'][index]
        annos.append(d)
    return annos


# ---- evaluation and the split driver --------------------------------------------------------------------------------------

def evaluation(det_annos, gt_annos, class_names):
    """Kitti2WaymoDataset.evaluation (l.382-392) with the ground truth passed in (`info['annos']` per frame):
    kitti_eval.get_official_eval_result on deep copies -> (result string, ret_dict)."""
    from . import kitti_eval
    return kitti_eval.get_official_eval_result(copy.deepcopy(gt_annos), copy.deepcopy(det_annos), class_names)


def evaluate_split(engine, infos, root_path, class_names, batch=2, output_path=None, _fov=None, _export=None, _evaluate=None):
    """Score `engine` on the frames of `infos` (kitti_infos_*.pkl entries: point_cloud.lidar_idx, image.image_shape, optionally annos):
    per batch of `batch` frames read `velodyne/<idx>.bin` ([n, 4] float32) and `calib/<idx>.txt` under `root_path`, FOV crop ->
    engine.forward -> generate_prediction_dicts; then evaluation against the infos' annos. No image file is read.
    -> (result_str, ret_dict, annos); (None, {}, annos) when the infos carry no annos, as the reference's evaluation does.
    Out of scope: info-file creation, label parsing, the road plane."""
    root_path = str(root_path)
    annos = []
    for at in range(0, len(infos), batch):
        part = infos[at:at + batch]
        ids = [info['point_cloud']['lidar_idx'] for info in part]
        calibs = [Calibration(os.path.join(root_path, 'calib', '%s.txt' % i)) for i in ids]
        shapes = [info['image']['image_shape'] for info in part]
        clouds = [np.fromfile(os.path.join(root_path, 'velodyne', '%s.bin' % i), dtype=np.float32).reshape(-1, 4) for i in ids]
        preds = engine.forward(fov_points(clouds, calibs, shapes, _fov=_fov))
        annos += generate_prediction_dicts({'frame_id': ids, 'calib': calibs, 'image_shape': shapes}, preds, class_names, output_path,
                                           _export=_export)
    if not infos or 'annos' not in infos[0]:
        return None, {}, annos
    result_str, ret_dict = (_evaluate or evaluation)(annos, [info['annos'] for info in infos], class_names)
    return result_str, ret_dict, annos
