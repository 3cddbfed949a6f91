"""numpy restatement of csrc/augment.hip (cpd_augment_scene, cpd_group_points_by_box), of the two in-box tests they sit
between, and -- through host_kernels() -- of cpd_amd.augmentor's host logic with the kernels replaced by these restatements,
so the whole augmentor runs on the CPU against tests/golden/augment.npz.

The rotation is the fused chain the kernel uses: x' = fma(y, -s, fl(x c)), y' = fma(y, c, fl(x s)) in float32 (torch's CPU
matmul for all but tiny N). fma32 below is exact: the product of two float32 is exact in float64, the sum's rounding error is
recovered by TwoSum, and a float64 sum that sits exactly half way between two float32 values is rounded by the error's sign.
"""
import contextlib
import pathlib
import pickle

import numpy as np
import torch

FLIP_X, FLIP_Y, ROT, SCALE = 0, 1, 2, 3
F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """float32 fma(a, b, c), correctly rounded, elementwise."""
    a, b, c = np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32)
    p = a.astype(F64) * b.astype(F64)                    # exact
    c64 = c.astype(F64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)                    # TwoSum: p + c = s + err exactly
    r = s.astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = r.astype(F64) - s
        other = np.nextafter(r, np.where(d > 0, -np.inf, np.inf).astype(F32))
        tie = (d != 0) & (np.abs(d) == np.abs(other.astype(F64) - s)) & (err != 0) & np.isfinite(s)
        lo, hi = np.minimum(r, other), np.maximum(r, other)
    return np.where(tie, np.where(err > 0, hi, lo), r).astype(F32)


def apply_ops(xyz, ops):
    """xyz [n, 3] float32 through ops = [(kind, p0, p1), ...]."""
    x, y, z = (xyz[:, 0].astype(F32).copy(), xyz[:, 1].astype(F32).copy(), xyz[:, 2].astype(F32).copy())
    for kind, p0, p1 in ops:
        if kind == FLIP_X:
            y = -y
        elif kind == FLIP_Y:
            x = -x
        elif kind == ROT:
            c, s = F32(p0), F32(p1)
            nx = fma32(y, -s, x * c)
            ny = fma32(y, c, x * s)
            x, y = nx, ny
        elif kind == SCALE:
            f = F32(p0)                                  # points[:, :3] *= Python float: a float32 product
            x, y, z = x * f, y * f, z * f
        else:
            raise ValueError(kind)
    return np.stack([x, y, z], 1)


def points_in_boxes_cpu(points, boxes):
    """check_pt_in_box3d_cpu (roiaware_pool3d.cpp:128-168): mask [k, n], MARGIN (float)1e-2, comparisons in double."""
    pts = np.asarray(points, F32)
    bx = np.asarray(boxes, F32).reshape(-1, 7)
    out = np.zeros((bx.shape[0], pts.shape[0]), bool)
    margin = F64(F32(1e-2))
    for k, q in enumerate(bx):
        ca, sa = F32(np.cos(F64(-q[6]))), F32(np.sin(F64(-q[6])))
        with np.errstate(invalid="ignore"):
            zok = ~(np.abs(pts[:, 2] - q[2]).astype(F64) > F64(q[5]) / 2.0)
            sx, sy = pts[:, 0] - q[0], pts[:, 1] - q[1]
            lx = (sx * ca + sy * (-sa)).astype(F32)
            ly = (sx * sa + sy * ca).astype(F32)
            out[k] = zok & (np.abs(lx).astype(F64) < F64(q[3]) / 2.0 + margin) & (np.abs(ly).astype(F64) < F64(q[4]) / 2.0 + margin)
    return out


def box_face_clearance(points, boxes, margin):
    """Smallest distance of any point to a face plane of any (margin-grown) box whose other two tests it passes loosely: the
    golden maker asserts it is far above a float32 ulp, so no in-box decision hangs on the last bit of a cos / sin."""
    pts = np.asarray(points, F64)
    best = np.inf
    for q in np.asarray(boxes, F64).reshape(-1, 7):
        ca, sa = np.cos(-q[6]), np.sin(-q[6])
        sx, sy = pts[:, 0] - q[0], pts[:, 1] - q[1]
        d = np.stack([np.abs(sx * ca - sy * sa) - (q[3] / 2 + margin), np.abs(sx * sa + sy * ca) - (q[4] / 2 + margin),
                      np.abs(pts[:, 2] - q[2]) - q[5] / 2], 1)
        near = (d < 0.05).all(1)
        if near.any():
            best = min(best, float(np.abs(d[near]).min()))
    return best


def points_in_boxes_gpu(points, boxes, margin=1e-5):
    """points_in_boxes_kernel (roiaware_pool3d_kernel.cu:23-35, 313-336): first containing box or -1, MARGIN 1e-5, float32."""
    pts = np.asarray(points, F32)
    bx = np.asarray(boxes, F32).reshape(-1, 7)
    out = np.full(pts.shape[0], -1, np.int32)
    for k in range(bx.shape[0] - 1, -1, -1):
        q = bx[k]
        hx, hy, hz = F32(F64(q[3]) / 2.0 + F64(F32(margin))), F32(F64(q[4]) / 2.0 + F64(F32(margin))), F32(F64(q[5]) / 2.0)
        ca, sa = np.cos(-q[6]).astype(F32), np.sin(-q[6]).astype(F32)
        sx, sy = pts[:, 0] - q[0], pts[:, 1] - q[1]
        lx = (sx * ca + sy * (-sa)).astype(F32)
        ly = (sx * sa + sy * ca).astype(F32)
        inside = ~(np.abs(pts[:, 2] - q[2]) > hz) & (np.abs(lx) < hx) & (np.abs(ly) < hy)
        out[inside] = k
    return out


def augment_scene(scene, ops=(), limit_range=None, obj_base=None, obj_start=None, obj_count=None, obj_centre=None, boxes=None):
    """cpd_augment_scene on numpy arrays: the kept rows [n_out, c]."""
    scene = np.asarray(scene, F32)
    c = scene.shape[1]
    rows = []
    k_obj = 0 if obj_start is None else len(obj_start)
    for s in range(k_obj):
        seg = np.asarray(obj_base, F32)[int(obj_start[s]):int(obj_start[s]) + int(obj_count[s]), :c].copy()
        seg[:, :3] = (seg[:, :3].astype(F64) + np.asarray(obj_centre[s], F64)[None, :]).astype(F32)
        rows.append(seg)
    if boxes is not None and len(boxes) and scene.shape[0]:
        scene = scene[~points_in_boxes_cpu(scene[:, :3], boxes).any(0)]
    rows.append(scene)
    pts = np.concatenate(rows, 0)
    pts[:, :3] = apply_ops(pts[:, :3], ops)
    if limit_range is not None:
        r = np.asarray(limit_range, F32)
        with np.errstate(invalid="ignore"):
            pts = pts[(pts[:, 0] >= r[0]) & (pts[:, 0] <= r[3]) & (pts[:, 1] >= r[1]) & (pts[:, 1] <= r[4])]
    return pts


def group_points_by_box(points, box_idx, centres):
    """cpd_group_points_by_box on numpy arrays: (rows [n_in_boxes, c], offsets [k + 1])."""
    points, box_idx = np.asarray(points, F32), np.asarray(box_idx)
    centres = np.asarray(centres, F64).reshape(-1, 3)
    k = centres.shape[0]
    valid = np.nonzero((box_idx >= 0) & (box_idx < k))[0]
    order = valid[np.argsort(box_idx[valid], kind="stable")]
    rows = points[order].copy()
    b = box_idx[order]
    if len(rows):
        rows[:, :3] = (rows[:, :3].astype(F64) - centres[b]).astype(F32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=k))]).astype(np.int32)
    return rows, offsets


def create_database(infos, save_path, used_classes, get_lidar, split="train"):
    """CPU transcription of create_track_groundtruth_database (waymo_unsupervised_dataset.py:653-754), the GPU in-box test
    replaced by points_in_boxes_gpu above. Writes the files; returns the dbinfos."""
    save_path = pathlib.Path(save_path)
    gt_path_name = pathlib.Path("pcdet_gt_track_database_%s_cp" % split)
    database_save_path = save_path / gt_path_name
    database_save_path.mkdir(parents=True, exist_ok=True)
    all_db_infos = {c: [] for c in used_classes}
    for cls_name in used_classes:
        for k in range(len(infos)):
            if cls_name == "Vehicle" and k % 10 != 0:
                continue
            if cls_name == "Pedestrian" and k % 5 != 0:
                continue
            info = infos[k]
            sequence_name, sample_idx = info["point_cloud"]["lidar_sequence"], info["point_cloud"]["sample_idx"]
            points = get_lidar(sequence_name, sample_idx)
            if len(info["outline_cls"]) == 0:
                continue
            names, gt_boxes, obj_ids = np.array(info["outline_cls"]), np.array(info["outline_box"]), np.array(info["outline_ids"])
            mask = names == cls_name
            names, gt_boxes, obj_ids = names[mask], gt_boxes[mask], obj_ids[mask]
            if gt_boxes.shape[0] == 0:
                continue
            idx = points_in_boxes_gpu(points[:, 0:3], gt_boxes[:, 0:7])
            for i in range(gt_boxes.shape[0]):
                filename = "%s_%s.bin" % (names[i], obj_ids[i])
                filepath = database_save_path / sequence_name / str(sample_idx) / filename
                gt_points = points[idx == i]
                gt_points[:, :3] -= gt_boxes[i, :3]
                if gt_points.shape[0] <= 5:
                    continue
                filepath.parent.mkdir(parents=True, exist_ok=True)
                with open(filepath, "wb") as f:
                    gt_points.tofile(f)
                all_db_infos[cls_name].append({
                    "name": cls_name, "path": str(gt_path_name / sequence_name / str(sample_idx) / filename),
                    "sequence_name": sequence_name, "seq_idx": sequence_name, "image_idx": sample_idx, "sample_idx": sample_idx,
                    "gt_idx": i, "ob_idx": obj_ids[i], "box3d_lidar": gt_boxes[i], "num_points_in_gt": gt_points.shape[0],
                    "pose": info["pose"], "difficulty": 1, "labeling_method_dict": ["unlabeled"]})
    with open(save_path / ("pcdet_waymo_track_dbinfos_%s_cp.pkl" % split), "wb") as f:
        pickle.dump(all_db_infos, f)
    return all_db_infos


@contextlib.contextmanager
def host_kernels():
    """cpd_amd.augmentor with its three device calls replaced by the restatements above (host tensors in, host tensors out):
    the module's host logic -- queues, sampler bookkeeping, box arithmetic, database writer -- then runs on the CPU."""
    from cpd_amd import augmentor as A
    from cpd_amd import prefilter

    def t2n(t):
        return None if t is None else (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))

    def aug(scene, ops=(), limit_range=None, obj_base=None, obj_start=None, obj_count=None, obj_centre=None, boxes=None):
        return torch.from_numpy(augment_scene(t2n(scene), ops, limit_range, t2n(obj_base), obj_start, obj_count, obj_centre,
                                              t2n(boxes)))

    def grp(points, box_idx, centres):
        rows, off = group_points_by_box(t2n(points), t2n(box_idx), centres)
        n = points.shape[0]
        full = np.zeros((n, points.shape[1]), F32)
        full[:len(rows)] = rows
        return torch.from_numpy(full), torch.from_numpy(off)

    def pib(points, boxes, margin=1e-5):
        return torch.from_numpy(points_in_boxes_gpu(t2n(points[0]), t2n(boxes[0]), margin))[None]

    saved = (A.augment_scene, A.group_points_by_box, prefilter.points_in_boxes_gpu)
    A.augment_scene, A.group_points_by_box, prefilter.points_in_boxes_gpu = aug, grp, pib
    try:
        yield A
    finally:
        A.augment_scene, A.group_points_by_box, prefilter.points_in_boxes_gpu = saved


# ---- the golden drive (shared by the maker and the tests, which rebuild the inputs from the seed) ---------------------------
SEQ = "segment-97531_augment"
CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
PCR = [-30.0, -30.0, -2.0, 30.0, 30.0, 4.0]        # inside the drive's 55 m object ring: pasted objects straddle it
EMPTY_FRAME = 3
N_FRAMES = 11


def sampler_config(sample_groups=("Vehicle:9", "Pedestrian:9", "Cyclist:10")):
    return dict(NAME="gt_sampling", USE_ROAD_PLANE=False, DB_INFO_PATH=["pcdet_waymo_track_dbinfos_train_cp.pkl"],
                PREPARE=dict(filter_by_min_points=["Vehicle:5", "Pedestrian:5", "Cyclist:5"], filter_by_difficulty=[-1]),
                SAMPLE_GROUPS=list(sample_groups), NUM_POINT_FEATURES=5, REMOVE_EXTRA_WIDTH=[0.0, 0.0, 0.0], LIMIT_WHOLE_SCENE=True)


def augmentor_config(with_sampling=True, with_rotation=True):
    lst = [sampler_config()] if with_sampling else []
    lst += [dict(NAME="random_world_flip", ALONG_AXIS_LIST=["x", "y"] if not with_rotation else ["x"])]
    if with_rotation:
        lst += [dict(NAME="random_world_rotation", WORLD_ROT_ANGLE=[-0.78539816, 0.78539816])]
    lst += [dict(NAME="random_world_scaling", WORLD_SCALE_RANGE=[0.95, 1.05])]
    return dict(DISABLE_AUG_LIST=["placeholder"], AUG_CONFIG_LIST=lst)


TEST_VIEWS = [(0, "None"), (0.39269908169872414, "None"), (-0.39269908169872414, "None"),
              (0, "x"), (0.39269908169872414, "x"), (-0.39269908169872414, "x")]


def test_view_config(rot, axis):
    return [dict(NAME="world_rotation", WORLD_ROT=rot), dict(NAME="world_flip", ALONG_AXIS=axis),
            dict(NAME="world_scaling", WORLD_SCALE=1)]


def drive(seed):
    """(frames, infos): N_FRAMES float32 clouds [n, 5] of a few thousand points (cpd_amd.synthetic.outline_scene, thinned) and
    OYSTER-style infos with hand-placed outline_box / outline_ids / outline_cls: the scene's own objects, jittered. Frame
    EMPTY_FRAME carries no labels at all."""
    from cpd_amd import synthetic
    rng = np.random.default_rng(seed + 4100)
    frames, infos = [], []
    for k in range(N_FRAMES):
        cloud = synthetic.outline_scene(seed * 100 + k, np.float32, n_az=120, n_vehicles=9, n_pedestrians=7, n_cyclists=5,
                                        n_clutter=3)
        objs = synthetic.outline_scene.last_objects
        boxes, ids, cls = [], [], []
        for j, (ctr, size, yaw, name) in enumerate(objs):
            if name not in CLASSES:
                continue
            boxes.append([ctr[0] + rng.normal(0, 0.05), ctr[1] + rng.normal(0, 0.05), ctr[2], size[0] * 1.08, size[1] * 1.08,
                          size[2] * 1.05, yaw + rng.normal(0, 0.02)])
            ids.append(j)
            cls.append(name)
        if k == EMPTY_FRAME:
            boxes, ids, cls = [], [], []
        pose = np.eye(4)
        pose[0, 3] = 0.35 * k
        infos.append(dict(point_cloud=dict(lidar_sequence=SEQ, sample_idx=k), pose=pose,
                          outline_box=np.array(boxes, np.float64).reshape(-1, 7), outline_ids=np.array(ids, np.int64),
                          outline_cls=np.array(cls, dtype=str) if cls else np.empty((0,), dtype=str)))
        frames.append(np.ascontiguousarray(cloud.astype(np.float32)))
    return frames, infos


def frame_labels(infos, f, keep_every=2):
    """The gt_boxes / gt_names training frame f carries into the augmentor (float32 boxes, as the dataset hands them over):
    every `keep_every`-th pseudo-label of the frame, so that the sampler has room to paste, and -- planted -- the first two
    labels of every class of frame 0, moved by (0.3, 0.2) m: the database objects cut from those boxes collide with them when
    they are sampled, so every class has rejected samples. Frame EMPTY_FRAME carries nothing."""
    info = infos[f]
    b = np.asarray(info["outline_box"], np.float32).reshape(-1, 7)[::keep_every].copy()
    n = np.asarray(info["outline_cls"])[::keep_every].copy()
    if f == EMPTY_FRAME:
        return b, n
    b0, n0 = np.asarray(infos[0]["outline_box"], np.float32), np.asarray(infos[0]["outline_cls"])
    for c in CLASSES:
        rows = np.nonzero(n0 == c)[0][:2]
        planted = b0[rows].copy()
        planted[:, 0] += np.float32(0.3)
        planted[:, 1] += np.float32(0.2)
        b = np.concatenate([b, planted], 0)
        n = np.concatenate([n, n0[rows]], 0)
    return b, n


def digest(frames, infos):
    import hashlib
    h = hashlib.sha256()
    for f, i in zip(frames, infos):
        h.update(np.ascontiguousarray(f).tobytes())
        h.update(np.ascontiguousarray(i["outline_box"]).tobytes())
    return h.hexdigest()


# ---- what the tests share: the golden's inputs rebuilt, its database on disk, and the comparisons ---------------------------
def rebuild(z):
    frames, infos = drive(int(z["seed"]))
    assert digest(frames, infos) == str(z["digest"]), "the drive rebuilt from the seed is not the golden's input"
    return frames, infos


def golden_dbinfos(z, infos):
    """The dbinfos the golden's database has, class by class, from its flattened arrays."""
    db = {c: [] for c in CLASSES}
    for i in range(len(z["db_path"])):
        sample_idx = int(z["db_sample_idx"][i])
        db[str(z["db_name"][i])].append({
            "name": str(z["db_name"][i]), "path": str(z["db_path"][i]), "sequence_name": SEQ, "seq_idx": SEQ, "image_idx": sample_idx,
            "sample_idx": sample_idx, "gt_idx": int(z["db_gt_idx"][i]), "ob_idx": z["db_ob_idx"][i], "box3d_lidar": z["db_box"][i],
            "num_points_in_gt": int(z["db_num"][i]), "pose": infos[sample_idx]["pose"], "difficulty": 1,
            "labeling_method_dict": ["unlabeled"]})
    return db


def write_golden_database(z, infos, root):
    root = pathlib.Path(root)
    for i, path in enumerate(z["db_path"]):
        f = root / str(path)
        f.parent.mkdir(parents=True, exist_ok=True)
        z["db_rows"][int(z["db_off"][i]):int(z["db_off"][i + 1])].tofile(str(f))
    with open(root / "pcdet_waymo_track_dbinfos_train_cp.pkl", "wb") as f:
        pickle.dump(golden_dbinfos(z, infos), f)


def assert_xyz_close(got, ref, what, rotated=True):
    """x, y within 2^-20 max(1, hypot(x_ref, y_ref)) where they went through a rotation: three roundings of <= 2^-24 relative on
    terms bounded by the radius, on each side, plus one ulp of cos / sin. Without a rotation x, y are the same bits. z is
    always the same bits: paste offset, flips and the float32 scale product are exact contracts."""
    assert np.asarray(got).shape == np.asarray(ref).shape, "%s: %s rows, the reference has %s" % (what, np.asarray(got).shape, np.asarray(ref).shape)
    if not rotated:
        assert np.asarray(got, F32).tobytes() == np.asarray(ref, F32).tobytes(), "%s: not the same bits without a rotation" % what
        return
    if np.asarray(ref).shape[1] > 2:
        assert np.asarray(got, F32)[:, 2].tobytes() == np.asarray(ref, F32)[:, 2].tobytes(), "%s: z differs" % what
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    bound = 2.0 ** -20 * np.maximum(1.0, np.hypot(ref[:, 0], ref[:, 1]))
    err = np.abs(got[:, :2] - ref[:, :2]).max(1) if len(ref) else np.zeros(0)
    print("%s: max xy error %.3e (bound %.3e at that row)" % (what, err.max() if len(err) else 0, bound[err.argmax()] if len(err) else 0))
    assert (err <= bound).all(), "%s: xy error %.3e" % (what, (err - bound).max())


def rest_digest(points):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(np.asarray(points)[:, 3:]).tobytes()).hexdigest()


def check_boxes(got, ref, what, rotated=True):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, ref.shape, ref.dtype)
    assert_xyz_close(got[:, :2], ref[:, :2], what + " centres", rotated)
    assert np.array_equal(got[:, 2:], ref[:, 2:]), what + ": a column other than x, y differs"


def to_host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def replay_scenes(A, z, frames, infos, root, device, resident=False, prepare=False):
    """The golden's scenes through cpd_amd.augmentor (module A, possibly under host_kernels): yields (scene index, the output
    dict with host points, the database paths of the objects it pasted, the permutation drawn by prepare_train_points or None)."""
    aug = A.DataAugmentor(pathlib.Path(root), augmentor_config(), CLASSES, logger=None, num_frames=1,
                          dataset_cfg=dict(current_label_method="unlabeled"), device=device, resident=resident)
    sampler = aug.data_augmentor_queue[0]
    for si, (f, sd) in enumerate(zip(z["scenes"], z["scene_seeds"])):
        gt_boxes, gt_names = frame_labels(infos, int(f))
        np.random.seed(int(sd))
        d = dict(points=torch.from_numpy(frames[int(f)].copy()).to(device), gt_boxes=gt_boxes.copy(), gt_names=gt_names.copy())
        perm = None
        if prepare:
            drawn, orig = [], np.random.permutation

            def rec(n):
                p = orig(n)
                if isinstance(n, (int, np.integer)):
                    drawn.append(p)
                return p

            np.random.permutation = rec
            try:
                mark = len(drawn)
                d = A.prepare_train_points(d, z["pcr"], True, shuffle=True, augmentor=aug)
            finally:
                np.random.permutation = orig
            perm = drawn[-1]
            assert mark == 0
        else:
            d = aug.forward(d)
        d["points"] = to_host(d["points"])
        yield si, d, [x["path"] for x in sampler.last_sampled], perm


NOROT_FRAME, NOROT_SEEDS = 5, (19, 20)


def replay_unrotated(A, z, frames, infos, root, device):
    """The golden's scenes without a rotation (gt_sampling, flips along x and y, scaling) through module A: [(d, pasted)]."""
    aug = A.DataAugmentor(pathlib.Path(root), augmentor_config(with_rotation=False), CLASSES, logger=None, num_frames=1,
                          dataset_cfg=dict(current_label_method="unlabeled"), device=device)
    out = []
    for sd in NOROT_SEEDS:
        gt_boxes, gt_names = frame_labels(infos, NOROT_FRAME)
        np.random.seed(int(sd))
        d = aug.forward(dict(points=torch.from_numpy(frames[NOROT_FRAME].copy()).to(device), gt_boxes=gt_boxes, gt_names=gt_names))
        d["points"] = to_host(d["points"])
        out.append((d, [x["path"] for x in aug.data_augmentor_queue[0].last_sampled]))
    return out


def check_unrotated(z, runs):
    """No rotation: every coordinate of points and boxes is the reference's, bit for bit."""
    assert len(runs) == len(NOROT_SEEDS)
    for i, (d, pasted) in enumerate(runs):
        check_forward_scene(z, i, d, pasted, prefix="n", rotated=False)


def check_forward_scene(z, si, d, pasted, prefix="s", rotated=True):
    p = "%s%d_" % (prefix, si)
    assert pasted == [str(x) for x in z[p + "pasted"]], "scene %d: sampled objects differ" % si
    assert np.array_equal(np.asarray(d["gt_names"], dtype=str), z[p + "gt_names"])
    assert ("valid_noise" in d) == bool(z[p + "has_valid_noise"])
    if "valid_noise" in d:
        assert np.array_equal(d["valid_noise"], z[p + "valid_noise"])
    assert np.array_equal(np.asarray(d["aug_param"], F64), z[p + "aug_param"]), "scene %d: aug_param" % si
    assert "calib" not in d and "road_plane" not in d
    assert str(d["points"].dtype) == str(z[p + "dtype"])
    assert_xyz_close(d["points"][:, :3], z[p + "xyz"], "scene %s%d points" % (prefix, si), rotated)
    assert rest_digest(d["points"]) == str(z[p + "rest"]), "scene %d: columns >= 3 differ" % si
    check_boxes(d["gt_boxes"], z[p + "gt_boxes"], "scene %s%d gt_boxes" % (prefix, si), rotated)


def check_prepared_scene(z, si, d, pasted, perm):
    import hashlib
    p = "s%d_" % si
    assert pasted == [str(x) for x in z[p + "pasted"]], "scene %d: sampled objects differ" % si
    n_all = len(z[p + "xyz"])
    mask = np.unpackbits(z[p + "mask"])[:n_all].astype(bool)
    assert len(perm) == int(z[p + "n_masked"]) == int(mask.sum()), "scene %d: %d rows in range, the reference has %d" % (si, len(perm), mask.sum())
    assert hashlib.sha256(np.asarray(perm, np.int64).tobytes()).hexdigest() == str(z[p + "perm"]), "scene %d: permutation differs" % si
    assert_xyz_close(d["points"][:, :3], z[p + "xyz"][mask][perm], "scene %d prepared points" % si)
    assert rest_digest(d["points"]) == str(z[p + "rest_prepared"]), "scene %d: columns >= 3 differ after mask and shuffle" % si
    bmask = z[p + "box_mask"]
    check_boxes(d["gt_boxes"], z[p + "gt_boxes"][bmask], "scene %d prepared gt_boxes" % si)
    assert np.array_equal(np.asarray(d["gt_names"], dtype=str), z[p + "gt_names"][bmask])
    if bool(z[p + "has_valid_noise"]):
        assert np.array_equal(d["valid_noise"], z[p + "valid_noise"][bmask])
    assert np.array_equal(np.asarray(d["aug_param"], F64), z[p + "aug_param"])


def check_database(z, infos, db, root):
    ref = golden_dbinfos(z, infos)
    with open(root / "pcdet_waymo_track_dbinfos_train_cp.pkl", "rb") as f:
        assert sorted(pickle.load(f).keys()) == sorted(ref.keys())
    files = sorted(str(p.relative_to(root)) for p in root.rglob("*.bin"))
    assert files == sorted(str(p) for p in z["db_path"])
    for i, path in enumerate(z["db_path"]):
        got = np.fromfile(str(root / str(path)), np.float32)
        want = z["db_rows"][int(z["db_off"][i]):int(z["db_off"][i + 1])].reshape(-1)
        assert got.tobytes() == want.tobytes(), path
    for c in CLASSES:
        assert len(db[c]) == len(ref[c]), c
        for g, r in zip(db[c], ref[c]):
            assert sorted(g.keys()) == sorted(r.keys())
            for key in r:
                if key in ("box3d_lidar", "pose"):
                    assert np.array_equal(g[key], r[key]) and np.asarray(g[key]).dtype == np.asarray(r[key]).dtype, key
                else:
                    assert g[key] == r[key], key
