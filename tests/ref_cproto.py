"""Numpy / scipy restatement of the first stage of CPD's C_PROTO refiner (cpd/unsupervised_core/c_proto_refine.py:65-195
compute_css_score_and_raw_proto, with outline_utils.py smooth_points, compute_confidence, hierarchical_occupancy_score,
KL_entropy_score and points_rigid_transform), stage by stage as cpd_amd.cproto computes it.

Where it departs from the letter of the reference, on purpose:
  * the ground step is tests/ref_outline.py's: ground_removal's np.argsort made stable (the canonical order);
  * compute_confidence's np.linalg.inv(trans_mat) of the float32 box transform is the closed form in float64, divided by
    c*c + s*s and rounded to float32, and the product with it is ((x*m00 + y*m01) + z*m02) + m03, unfused, in float64 (the
    reference leaves both to LAPACK / BLAS). make_golden_cproto.py flags the boxes where that changes a cell count.
scipy is imported inside smooth_mask only (the GPU tests use the rest without it)."""
import copy

import numpy as np

import ref_outline as RO

CLASSES = ('Vehicle', 'Pedestrian', 'Cyclist')


def get(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def ground_cfg(cfg):
    """The OutlineFitter arguments C_PROTO.__init__ passes (GroundMin in place of ground_min_threshold)."""
    g = get(cfg, "GeneratorConfig")
    out = {k: get(g, k) for k in ("sensor_height", "ground_min_distance", "cluster_dis", "cluster_min_points",
                                  "discard_max_height")}
    out["ground_min_threshold"] = get(get(cfg, "RefinerConfig"), "GroundMin")
    return out


def presize(box, name, predefined):
    """l.111-118: the Pedestrian / Cyclist size overwrite (a copy)."""
    box = np.array(box, np.float64)
    if name == 'Pedestrian':
        box[3:5] = np.array(predefined['Pedestrian'])[0:2]
    if name == 'Cyclist':
        box[4] = np.array(predefined['Cyclist'])[1]
    return box


def crop_mask(xyz, box):
    dis = np.sqrt(np.sum((xyz[:, 0:2] - box[0:2]) ** 2, -1))
    return dis < (max(box[3], box[4]))


def smooth_mask(xyz, rad=0.2):
    from scipy.spatial import cKDTree
    if len(xyz) == 0:
        return np.zeros(0, bool)
    num = cKDTree(xyz[:, 0:3]).query_ball_point(xyz[:, 0:3], r=rad, return_length=True)
    return num > 3


def smooth_mask_brute(xyz, rad=0.2):
    """The same count by the float64 expression the kernel evaluates (small inputs)."""
    p = xyz[:, 0:3].astype(np.float64)
    d = p[:, None, :] - p[None]
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= rad * rad).sum(1) > 3


def inv_rows32(box):
    """Rows 0 and 1 of the inverse of compute_confidence's float32 trans_mat: closed form in float64, rounded to float32."""
    c, s = np.float32(np.cos(box[6])), np.float32(np.sin(box[6]))
    x, y = np.float32(box[0]), np.float32(box[1])
    c, s, x, y = np.float64(c), np.float64(s), np.float64(x), np.float64(y)
    d = c * c + s * s
    m = np.array([c / d, s / d, 0.0, -(c * x + s * y) / d, -s / d, c / d, 0.0, (s * x - c * y) / d])
    return m.astype(np.float32)


def box_frame_xy(points, m):
    p = np.asarray(points, np.float64)
    m = np.asarray(m, np.float32).astype(np.float64)
    X = ((p[:, 0] * m[0] + p[:, 1] * m[1]) + p[:, 2] * m[2]) + m[3]
    Y = ((p[:, 0] * m[4] + p[:, 1] * m[5]) + p[:, 2] * m[6]) + m[7]
    return X, Y


def occupancy(points, box, parts):
    """compute_confidence's valid_vol (the number of cells with more than one point)."""
    l, w = box[3], box[4]
    X, Y = box_frame_xy(points, inv_rows32(box))
    delta_l = l / parts
    delta_w = w / parts
    valid_vol = 0
    for i in range(parts):
        for j in range(parts):
            mask = (-l / 2 + i * delta_l <= X) * (X < -l / 2 + (i + 1) * delta_l) * \
                   (-w / 2 + j * delta_w <= Y) * (Y < -w / 2 + (j + 1) * delta_w)
            if mask.sum() > 1:
                valid_vol += 1
    return valid_vol


def KL_entropy_score(x, y, max_dif=0.05):
    KL = 0.0
    for i in range(len(x)):
        KL += x[i] * np.log(x[i] / y[i])
    if KL > max_dif:
        KL = max_dif
    return (max_dif - KL) / max_dif


def css_from_occ(occ, box, name, css_cfg):
    """CSS.compute_css (l.20-41) with the cell counts given."""
    max_dis, parts = get(css_cfg, "MaxDis"), get(css_cfg, "MLOParts")
    dis_dis = np.linalg.norm(box[0:3])
    if dis_dis > max_dis:
        dis_dis = max_dis
    dis_score = 1 - dis_dis / max_dis
    all_confi = 0
    for o, part in zip(occ, parts):
        all_confi += int(o) / (part ** 2)
    mlo_score = all_confi / len(parts)
    new_box = copy.deepcopy(box)
    this_size_norm = new_box[3:6] / new_box[3:6].sum()
    this_temp_norm = np.array(get(css_cfg, "PredifinedSize")[name])
    this_temp_norm = this_temp_norm / this_temp_norm.sum()
    size_score = KL_entropy_score(this_size_norm, this_temp_norm)
    weights = np.array(get(css_cfg, "CSS_weight"))
    weights = np.array(weights) / np.sum(weights)
    return dis_score * weights[0] + mlo_score * weights[1] + size_score * weights[2]


def segment(xyz, box, cfg, brute=False):
    """One (frame, box) pair after the size overwrite: every stage's output as a dict. xyz [N, 3] float16 / float32."""
    gcfg = ground_cfg(cfg)
    parts = get(get(get(cfg, "RefinerConfig"), "CSSConfig"), "MLOParts")
    box = np.asarray(box, np.float64)
    out = {}
    cm = crop_mask(xyz, box)
    out["crop_src"] = np.nonzero(cm)[0]
    low = xyz[cm]
    dens = (smooth_mask_brute if brute else smooth_mask)(low) if len(low) else np.zeros(0, bool)
    out["dens_mask"] = dens
    low_src = out["crop_src"][dens]
    low = low[dens]
    if len(low) > 0:
        z_min = min(low[:, 2])
    else:
        z_min = box[2] - box[5] / 2
    z_max = box[2] + box[5] / 2
    h = z_max - z_min
    if h < 1.3:
        h = 1.3
    z = h / 2 + z_min
    out["z_min"] = float(z_min)
    out["new_box"] = np.array([box[0], box[1], z, box[3], box[4], h, box[6]])
    out["had_points"] = len(low) > 0
    out["filt_src"] = np.zeros(0, np.int64)
    out["ng_src"] = np.zeros(0, np.int64)
    out["labels"] = np.zeros(0, np.int64)
    out["best_label"], out["best_count"], out["occ"] = -1, 0, np.zeros(len(parts), np.int32)
    out["cluster"], out["cluster_src"] = np.zeros((0, 3)), np.zeros(0, np.int64)
    if len(low) > 0:
        mask = (low[:, 2] > z_min + 0.2) * (low[:, 2] < z_max)
        low, low_src = low[mask], low_src[mask]
        out["filt_src"] = low_src
        ng, src = RO.remove_ground(low, gcfg, return_index=True)
        out["ng_src"] = low_src[src]
        if len(ng) > 10:
            labels = RO.dbscan_labels(ng, gcfg["cluster_dis"])
            out["labels"] = labels
            best, best_n = -1, 0
            for i in range(int(labels.max()) + 1):
                pts = ng[labels == i]
                if len(pts) > gcfg["cluster_min_points"] and pts[:, 2].max() < gcfg["discard_max_height"] and len(pts) > best_n:
                    best, best_n = i, len(pts)
            if best >= 0:
                out["best_label"], out["best_count"] = best, best_n
                out["cluster"] = ng[labels == best]
                out["cluster_src"] = out["ng_src"][labels == best]
                out["occ"] = np.array([occupancy(out["cluster"], out["new_box"], p) for p in parts], np.int32)
    return out


def points_rigid_transform(cloud, pose):
    cloud = np.array(cloud)
    if cloud.shape[0] == 0:
        return cloud
    mat = np.ones(shape=(cloud.shape[0], 4), dtype=np.float32)
    mat[:, 0:3] = cloud[:, 0:3]
    T = np.array((np.asarray(pose) @ mat.astype(np.float64).T).T, dtype=np.float32)
    return T[:, 0:3]


def run_sequence(frames, infos, cfg, seq_id, on_segment=None):
    """compute_css_score_and_raw_proto over frames (list of [N, >=3]) and the input info list: (infos, raw_proto_set).
    on_segment(i, box_id, seg_dict) sees every segment's stages."""
    infos = copy.deepcopy(infos)
    rcfg = get(cfg, "RefinerConfig")
    css_cfg = get(rcfg, "CSSConfig")
    predefined = get(css_cfg, "PredifinedSize")
    thresh = get(rcfg, "BasicProtoScoreThresh")
    raw = {c: {} for c in CLASSES}
    for i, info in enumerate(infos):
        boxes, cls, ids, pose = info['outline_box'], info['outline_cls'], info['outline_ids'], info['pose']
        score = np.zeros(shape=cls.shape)
        xyz = frames[i][:, 0:3]
        for b in range(len(boxes)):
            name = cls[b]
            if name not in raw:
                continue
            box = presize(boxes[b], name, predefined)
            boxes[b] = box
            seg = segment(xyz, box, cfg)
            if seg["best_label"] >= 0:
                seg["score"] = css_from_occ(seg["occ"], seg["new_box"], name, css_cfg)
                score[b] = seg["score"]
                boxes[b] = seg["new_box"]
                if seg["score"] > thresh[name]:
                    pid = int(str(seq_id) + str(ids[b]))
                    gp = points_rigid_transform([seg["new_box"][0:3]], pose)[0:, 0:3]
                    if pid in raw[name]:
                        pose_i = np.linalg.inv(raw[name][pid]['pose'][0])
                        pts = points_rigid_transform(points_rigid_transform(seg["cluster"], pose), pose_i)
                        e = raw[name][pid]
                        e['points'].append(pts), e['outline_box'].append(seg["new_box"]), e['pose'].append(pose)
                        e['score'].append(seg["score"]), e['global_position'].append(gp)
                    else:
                        raw[name][pid] = {'points': [seg["cluster"]], 'outline_box': [seg["new_box"]], 'pose': [pose],
                                          'score': [seg["score"]], 'global_position': [gp]}
            if on_segment is not None:
                on_segment(i, b, seg)
        info['outline_score'] = score
    return infos, raw
