"""Synthetic point clouds and boxes (build-owned, seeded) for parity tests and bench.py.

W-cloud: a 64-beam x 2650-azimuth spinning lidar (elevations -17.6..+2.4 deg, sensor 2 m above a
ground plane at z=0) ray-cast against the ground and 60 vertical cylinders/"buildings", clipped at
75 m, 2 cm range noise, sub-sampled to the requested number of returns (160 k = the Waymo-shape
config of BASELINE.json). Features [x, y, z, intensity, elongation] f32.
K-cloud: the same scene model restricted to the KITTI field of view, [x, y, z, intensity].
"""
import numpy as np

# Config W (tools/cfgs/dataset_configs/waymo_unsupervised/waymo_unsupervised_cproto.yaml:118,166-172)
WAYMO = dict(point_cloud_range=[-75.2, -75.2, -2.0, 75.2, 75.2, 4.0], voxel_size=[0.1, 0.1, 0.15],
             max_points_per_voxel=5, max_voxels=1000000, num_point_features=5)
# Config K (KITTI-shape, 0.05 m; height_compression.py:48 defaults)
KITTI = dict(point_cloud_range=[0.0, -40.0, -3.0, 70.4, 40.0, 1.0], voxel_size=[0.05, 0.05, 0.1],
             max_points_per_voxel=5, max_voxels=1000000, num_point_features=4)
# Config C1: KITTI range at 0.1 m voxels
KITTI_C1 = dict(point_cloud_range=[0.0, -40.0, -3.0, 70.4, 40.0, 1.0], voxel_size=[0.1, 0.1, 0.1],
                max_points_per_voxel=5, max_voxels=1000000, num_point_features=4)


def _raycast(rng, n_az, elev_deg, sensor_z, n_obj, max_range, fov=None):
    elev = np.deg2rad(np.linspace(elev_deg[0], elev_deg[1], 64))
    az = np.linspace(0.0, 2 * np.pi, n_az, endpoint=False)
    if fov is not None:
        az = np.linspace(fov[0], fov[1], n_az)
    e, a = np.meshgrid(elev, az, indexing="ij")
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], -1).reshape(-1, 3)
    t_best = np.full(d.shape[0], np.inf)
    dz = d[:, 2]
    tg = np.where(dz < -1e-6, -sensor_z / np.minimum(dz, -1e-6), np.inf)
    t_best = np.minimum(t_best, tg)
    # objects: vertical cylinders (cars/pedestrians) and a ring of large "buildings"
    n_small = n_obj - 12
    cx = np.concatenate([rng.uniform(-70, 70, n_small), 62 * np.cos(np.linspace(0, 2 * np.pi, 12, endpoint=False))])
    cy = np.concatenate([rng.uniform(-70, 70, n_small), 62 * np.sin(np.linspace(0, 2 * np.pi, 12, endpoint=False))])
    rad = np.concatenate([rng.uniform(0.5, 2.5, n_small), rng.uniform(6.0, 12.0, 12)])
    hgt = np.concatenate([rng.uniform(1.2, 3.5, n_small), rng.uniform(6.0, 14.0, 12)])
    keep = np.hypot(cx, cy) > rad + 3.0   # nothing on top of the sensor
    dxy = d[:, :2]
    a2 = (dxy ** 2).sum(1)
    for k in np.nonzero(keep)[0]:
        c = np.array([cx[k], cy[k]])
        b = -(dxy @ c)
        cc = c @ c - rad[k] ** 2
        disc = b * b - a2 * cc
        ok = disc > 0
        t = np.where(ok, (-b - np.sqrt(np.where(ok, disc, 0))) / a2, np.inf)
        z = sensor_z + t * dz
        t = np.where((t > 0.5) & (z >= 0.0) & (z <= hgt[k]), t, np.inf)
        t_best = np.minimum(t_best, t)
    hit = np.isfinite(t_best) & (t_best < max_range)
    t = t_best[hit] + rng.normal(0, 0.02, hit.sum())
    pts = d[hit] * t[:, None]
    pts[:, 2] += sensor_z
    return pts


def waymo_cloud(seed=0, n_points=160000, n_az=2650):
    """Waymo-shape cloud, [n_points, 5] f32 in scan order."""
    rng = np.random.default_rng(seed)
    while True:
        pts = _raycast(rng, n_az, (-17.6, 2.4), 2.0, 60, 75.0)
        if pts.shape[0] >= n_points:
            break
        n_az = int(n_az * 1.15) + 1   # denser azimuth sampling until enough returns
    if pts.shape[0] > n_points:
        sel = np.sort(rng.choice(pts.shape[0], n_points, replace=False))
        pts = pts[sel]
    out = np.empty((pts.shape[0], 5), np.float32)
    out[:, :3] = pts
    out[:, 3] = rng.uniform(0, 1, pts.shape[0])
    out[:, 4] = rng.uniform(0, 1, pts.shape[0])
    return out


def kitti_cloud(seed=0, n_points=20000):
    """KITTI-shape cloud (front field of view), [n_points, 4] f32."""
    rng = np.random.default_rng(seed + 1000)
    n_az = 900
    while True:
        pts = _raycast(rng, n_az, (-24.8, 2.0), 1.73, 40, 80.0, fov=(-np.pi / 4, np.pi / 4))
        m = (pts[:, 0] > 0) & (pts[:, 0] < 70.4) & (np.abs(pts[:, 1]) < 40)
        pts = pts[m]
        pts[:, 2] -= 1.73  # KITTI velodyne frame: ground at z = -1.73
        if pts.shape[0] >= n_points:
            break
        n_az = int(n_az * 1.2) + 1
    if pts.shape[0] > n_points:
        sel = np.sort(rng.choice(pts.shape[0], n_points, replace=False))
        pts = pts[sel]
    out = np.empty((pts.shape[0], 4), np.float32)
    out[:, :3] = pts
    out[:, 3] = rng.uniform(0, 1, pts.shape[0])
    return out


def random_boxes(seed, n, span=75.0, dup_frac=0.1):
    """NMS test boxes [n,7] + distinct scores: centres U(-span, span), dims LogNormal around
    (4.7, 2.1, 1.7), heading U(-pi, pi), 10 % near-duplicates."""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-span, span, (n, 2))
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3:6] = np.exp(rng.normal(0, 0.25, (n, 3))) * np.array([4.7, 2.1, 1.7])
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    k = int(n * dup_frac)
    if k:
        b[n - k:] = b[:k]
        b[n - k:, :2] += rng.normal(0, 0.25, (k, 2)).astype(np.float32)
        b[n - k:, 6] += rng.normal(0, 0.05, k).astype(np.float32)
    scores = (rng.permutation(n).astype(np.float32) + 1) / (n + 1)
    return b.astype(np.float32), scores


# PredifinedSize of waymo_unsupervised_cproto.yaml:85 (Vehicle, Pedestrian, Cyclist)
PREDEFINED_SIZE = np.array([[5.065, 1.86, 1.49], [1.0, 1.0, 2.0], [1.9, 0.85, 1.8]], np.float32)


def gt_boxes(seed, n=30, span=70.0):
    """Synthetic ground truth of the config-3 train step: [n, 8] =
    (x, y, z, dx, dy, dz, heading, class 1..3), centres uniform within +-span on the ground,
    sizes PredifinedSize x U(0.9, 1.1), heading U(-pi, pi)."""
    rng = np.random.default_rng(1000 + seed)
    cls = rng.integers(1, 4, n)
    dims = PREDEFINED_SIZE[cls - 1] * rng.uniform(0.9, 1.1, (n, 3)).astype(np.float32)
    b = np.zeros((n, 8), np.float32)
    b[:, 0:2] = rng.uniform(-span, span, (n, 2))
    b[:, 2] = dims[:, 2] / 2.0                         # resting on the ground plane z = 0
    b[:, 3:6] = dims
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    b[:, 7] = cls
    return b


# ---- KITTI-format annotations (kitti_common label dicts) for the evaluation ----------------------------------------
_KITTI_DIMS = {"Car": (3.9, 1.55, 1.65), "Van": (5.0, 2.1, 1.9), "Truck": (9.0, 3.2, 2.5), "Pedestrian": (0.8, 1.75, 0.6),
               "Person_sitting": (0.8, 1.2, 0.6), "Cyclist": (1.76, 1.7, 0.6)}
_KITTI_GT_NAMES = ["Car", "Car", "Car", "Pedestrian", "Pedestrian", "Cyclist", "Cyclist", "Van", "Person_sitting",
                   "DontCare", "Truck"]


def _kitti_image_box(loc, dims, rng):
    """A plausible 2-D box for a camera-frame object (pinhole, f = 720 px, principal point (620, 190)), clipped."""
    x, y, z = loc
    l, h, w = dims
    span = 720.0 * max(l, w) * 0.8 / z
    u, v_bot, hpx = 620.0 + 720.0 * x / z, 190.0 + 720.0 * y / z, 720.0 * h / z
    box = np.array([u - span / 2, v_bot - hpx, u + span / 2, v_bot]) + rng.normal(0, 1.0, 4)
    return np.clip(box, [0, 0, 0, 0], [1241, 374, 1241, 374])


def kitti_annos(n_frames, seed=0, max_gt=12, max_fp=4, p_empty_dt=0.05, p_empty_gt=0.05):
    """Seeded (gt_annos, dt_annos) lists in kitti_common's label-dict format (float64 arrays): Car / Pedestrian / Cyclist
    plus Van, Person_sitting, Truck and DontCare gts whose occlusion, truncation and 2-D heights span the three
    difficulty bins; detections are jittered gts (names kept, Van sometimes detected as Car) plus false positives, with
    two-decimal scores (ties) and valid alpha. Some frames have no gt, some no detection."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for _ in range(n_frames):
        n_gt = 0 if rng.random() < p_empty_gt else int(rng.integers(1, max_gt + 1))
        g = {k: [] for k in ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y")}
        d = {k: [] for k in ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y",
                             "score")}
        for _ in range(n_gt):
            name = _KITTI_GT_NAMES[int(rng.integers(len(_KITTI_GT_NAMES)))]
            if name == "DontCare":
                g["name"].append(name)
                g["truncated"].append(-1.0)
                g["occluded"].append(-1)
                g["alpha"].append(-10.0)
                u, v = rng.uniform(0, 1100), rng.uniform(120, 300)
                g["bbox"].append([u, v, u + rng.uniform(10, 140), v + rng.uniform(8, 70)])
                g["dimensions"].append([-1.0, -1.0, -1.0])
                g["location"].append([-1000.0, -1000.0, -1000.0])
                g["rotation_y"].append(-10.0)
                continue
            dims = np.array(_KITTI_DIMS[name]) * rng.uniform(0.85, 1.15, 3)
            loc = np.array([rng.uniform(-15, 15), rng.uniform(1.2, 2.2), rng.uniform(4, 70)])
            ry = rng.uniform(-np.pi, np.pi)
            bbox = _kitti_image_box(loc, dims, rng)
            g["name"].append(name)
            g["truncated"].append(float(rng.choice([0.0, 0.0, 0.1, 0.25, 0.4, 0.7])))
            g["occluded"].append(int(rng.choice([0, 0, 1, 2, 3])))
            g["alpha"].append(ry - np.arctan2(loc[0], loc[2]))
            g["bbox"].append(bbox)
            g["dimensions"].append(dims)
            g["location"].append(loc)
            g["rotation_y"].append(ry)
            if rng.random() < 0.8:
                scale = 0.04 * loc[2] / 10.0
                dloc = loc + rng.normal(0, [scale, 0.05, scale])
                ddims = dims * (1 + rng.normal(0, 0.06, 3))
                dry = ry + rng.normal(0, 0.12) + (np.pi if rng.random() < 0.05 else 0.0)
                dname = "Car" if name == "Van" and rng.random() < 0.5 else name
                d["name"].append(dname)
                d["bbox"].append(bbox + rng.normal(0, 2.0 + 30.0 / loc[2], 4))
                d["dimensions"].append(ddims)
                d["location"].append(dloc)
                d["rotation_y"].append(dry)
                d["alpha"].append(dry - np.arctan2(dloc[0], dloc[2]))
                d["score"].append(round(float(rng.uniform(0.05, 1.0)), 2))
        for _ in range(int(rng.integers(0, max_fp + 1))):
            name = ["Car", "Pedestrian", "Cyclist"][int(rng.integers(3))]
            dims = np.array(_KITTI_DIMS[name]) * rng.uniform(0.85, 1.15, 3)
            loc = np.array([rng.uniform(-15, 15), rng.uniform(1.2, 2.2), rng.uniform(4, 70)])
            ry = rng.uniform(-np.pi, np.pi)
            d["name"].append(name)
            d["bbox"].append(_kitti_image_box(loc, dims, rng))
            d["dimensions"].append(dims)
            d["location"].append(loc)
            d["rotation_y"].append(ry)
            d["alpha"].append(ry - np.arctan2(loc[0], loc[2]))
            d["score"].append(round(float(rng.uniform(0.05, 0.9)), 2))
        if rng.random() < p_empty_dt:
            d = {k: [] for k in d}
        n_dt = len(d["name"])
        d["truncated"] = [0.0] * n_dt
        d["occluded"] = [0] * n_dt
        gts.append(_kitti_dict(g))
        dts.append(_kitti_dict(d))
    return gts, dts


def _kitti_dict(a):
    out = {}
    for k, v in a.items():
        if k == "name":
            out[k] = np.array(v, dtype="<U14") if v else np.zeros(0, dtype="<U14")
        elif k == "occluded":
            out[k] = np.array(v, dtype=np.int64)
        elif k in ("bbox",):
            out[k] = np.array(v, dtype=np.float64).reshape(-1, 4)
        elif k in ("dimensions", "location"):
            out[k] = np.array(v, dtype=np.float64).reshape(-1, 3)
        else:
            out[k] = np.array(v, dtype=np.float64)
    return out


_WAYMO_SIZES = {"Vehicle": (4.6, 2.0, 1.6), "Pedestrian": (0.8, 0.7, 1.7), "Cyclist": (1.8, 0.7, 1.7)}


def waymo_infos(n_frames, seed=0, n_gt=60, n_pd=150):
    """Seeded (prediction_infos, gt_infos) in the format Dataset.evaluation hands cpd_amd.waymo_eval (lidar-frame centre
    boxes: call waymo_evaluation with fake_gt_infos=False): about n_gt ground truths per frame (Vehicle / Pedestrian /
    Cyclist, point counts spanning both levels and zero) and about n_pd predictions: jittered copies of four fifths of
    the ground truths, a second lower-scored copy of a third of them, and unrelated boxes for the rest."""
    rng = np.random.default_rng(seed)
    names = np.array(list(_WAYMO_SIZES))
    sizes = np.array([_WAYMO_SIZES[n] for n in names])
    pds, gts = [], []

    def boxes(kind, n):
        r, phi = rng.uniform(3, 75, n), rng.uniform(-np.pi, np.pi, n)
        dims = sizes[kind] * rng.uniform(0.85, 1.15, (n, 3))
        return np.column_stack([r * np.cos(phi), r * np.sin(phi), rng.uniform(-0.5, 1.5, n), dims, rng.uniform(-np.pi, np.pi, n)])

    for _ in range(n_frames):
        ng = int(rng.integers(max(1, n_gt - n_gt // 4), n_gt + n_gt // 4 + 1))
        kind = rng.choice(3, ng, p=[0.55, 0.35, 0.1])
        g = boxes(kind, ng)
        gts.append({"name": names[kind], "difficulty": np.zeros(ng, np.int32),
                    "num_points_in_gt": rng.choice([0, 3, 5, 12, 80, 400], ng, p=[0.03, 0.1, 0.07, 0.2, 0.3, 0.3]).astype(np.int64),
                    "gt_boxes_lidar": g.astype(np.float32)})
        hit = np.nonzero(rng.random(ng) < 0.8)[0]
        twice = hit[rng.random(len(hit)) < 0.33]
        src = np.concatenate([hit, twice])
        jit = g[src] + rng.normal(0, 1.0, (len(src), 7)) * np.array([0.12, 0.12, 0.05, 0.1, 0.05, 0.05, 0.06])
        score = np.concatenate([rng.uniform(0.3, 1.0, len(hit)), rng.uniform(0.02, 0.5, len(twice))])
        n_fp = max(0, int(rng.integers(n_pd - n_pd // 5, n_pd + n_pd // 5 + 1)) - len(src))
        fk = rng.choice(3, n_fp)
        pds.append({"name": np.concatenate([names[kind[src]], names[fk]]),
                    "score": np.concatenate([score, rng.uniform(0.01, 0.6, n_fp)]).astype(np.float32),
                    "boxes_lidar": np.concatenate([jit, boxes(fk, n_fp)]).astype(np.float32)})
    return pds, gts


# ---- pseudo-label scene (cpd_amd.outline) --------------------------------------------------------------------------------

def _ray_obb(d, sensor_z, c, size, yaw):
    """Entry distance of unit rays d [R, 3] from (0, 0, sensor_z) into the box (centre c, size (l, w, h), heading yaw); inf
    where missed (slab test in the box frame)."""
    cs, sn = np.cos(-yaw), np.sin(-yaw)
    o = np.array([-c[0], -c[1], sensor_z - c[2]])
    o = np.array([cs * o[0] - sn * o[1], sn * o[0] + cs * o[1], o[2]])
    db = np.stack([cs * d[:, 0] - sn * d[:, 1], sn * d[:, 0] + cs * d[:, 1], d[:, 2]], -1)
    half = np.asarray(size, np.float64) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (-half - o) / db
        t2 = (half - o) / db
    t1 = np.where(np.isnan(t1), -np.inf, t1)
    t2 = np.where(np.isnan(t2), np.inf, t2)
    tn = np.minimum(t1, t2).max(1)
    tf = np.maximum(t1, t2).min(1)
    return np.where((tn <= tf) & (tn > 0.5), tn, np.inf)


def outline_scene(seed=0, dtype=np.float16, n_az=2650, n_vehicles=14, n_pedestrians=10, n_cyclists=6, n_clutter=10):
    """A Waymo-shape frame for the pseudo-label generator (cpd_amd.outline): the waymo_cloud beam pattern (64 beams,
    -17.6..+2.4 deg, sensor 2 m above z = 0, 75 m range, 2 cm range noise) ray-cast against
      * ground with N(0, 2 cm) height noise and one sloped sector (azimuth 1.0..1.6 rad, rising 8 % beyond 15 m), so the
        ground fit breaks, restarts and skips bin gaps;
      * oriented boxes sized inside the config's Vehicle / Pedestrian / Cyclist ranges, low clutter 0.3..0.6 m high, one
        tall structure (8 m) and the waymo_cloud ring of 12 buildings.
    Returns [N, 5] of `dtype` (float16, as Waymo frames are saved, or float32): x, y, z, intensity, elongation.
    Points whose ground segment index would change under +-2 float32 ulp of atan2 are rotated about z in small steps until
    it does not (atan2 is the one projection op that is not reproducible bit for bit across libraries)."""
    dtype = np.dtype(dtype)
    if dtype not in (np.float16, np.float32):
        raise TypeError("outline_scene: float16 or float32")
    rng = np.random.default_rng(seed + 7000)
    sensor_z = 2.0
    elev = np.deg2rad(np.linspace(-17.6, 2.4, 64))
    az = np.linspace(0.0, 2 * np.pi, n_az, endpoint=False) + rng.uniform(0, 2 * np.pi / n_az)
    e, a = np.meshgrid(elev, az, indexing="ij")
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], -1).reshape(-1, 3)
    ce, dz = np.cos(e).reshape(-1), d[:, 2]
    azr = np.mod(a.reshape(-1), 2 * np.pi)
    # ground: flat z = 0, or z = s * (r - r0) in the sloped sector beyond r0
    t_flat = np.where(dz < -1e-6, -sensor_z / np.minimum(dz, -1e-6), np.inf)
    s, r0 = 0.08, 15.0
    sector = (azr > 1.0) & (azr < 1.6)
    with np.errstate(divide="ignore"):
        t_slope = (sensor_z + s * r0) / (s * ce - dz)
    slope_ok = sector & (t_slope > 0) & (t_slope * ce > r0)
    t_ground = np.where(slope_ok, t_slope, t_flat)
    t_best, is_ground = t_ground.copy(), np.isfinite(t_ground)

    def place(n, lo_r, hi_r):
        r = rng.uniform(lo_r, hi_r, n)
        ang = rng.uniform(0, 2 * np.pi, n)
        ang = np.where((ang > 0.9) & (ang < 1.7), ang + 1.0, ang)   # objects stay off the sloped sector
        return np.stack([r * np.cos(ang), r * np.sin(ang)], -1)

    objs = []
    for n, (l0, l1), (w0, w1), (h0, h1), rr in [(n_vehicles, (3.6, 5.2), (1.7, 2.2), (1.4, 2.1), (6, 55)),
                                                (n_pedestrians, (0.5, 0.8), (0.4, 0.7), (1.5, 1.9), (5, 35)),
                                                (n_cyclists, (1.6, 2.1), (0.6, 0.9), (1.5, 1.9), (5, 40)),
                                                (n_clutter, (0.6, 1.5), (0.5, 1.2), (0.3, 0.6), (5, 30)),
                                                (1, (3.0, 4.0), (3.0, 4.0), (8.0, 8.0), (20, 30))]:
        for xy in place(n, *rr):
            size = (rng.uniform(l0, l1), rng.uniform(w0, w1), rng.uniform(h0, h1))
            objs.append((np.array([xy[0], xy[1], size[2] / 2]), size, rng.uniform(-np.pi, np.pi)))
    for k in range(12):
        ang = 2 * np.pi * k / 12
        size = (rng.uniform(8, 14), rng.uniform(8, 14), rng.uniform(6, 14))
        objs.append((np.array([62 * np.cos(ang), 62 * np.sin(ang), size[2] / 2]), size, ang))
    names = ['Vehicle'] * n_vehicles + ['Pedestrian'] * n_pedestrians + ['Cyclist'] * n_cyclists + ['Dis_Small'] * n_clutter
    outline_scene.last_objects = [(c, size, yaw, name) for (c, size, yaw), name in zip(objs, names)]   # for cproto_sequence
    for c, size, yaw in objs:
        t = _ray_obb(d, sensor_z, c, size, yaw)
        closer = t < t_best
        t_best = np.where(closer, t, t_best)
        is_ground &= ~closer
    hit = np.isfinite(t_best) & (t_best < 75.0)
    t = t_best[hit] + rng.normal(0, 0.02, hit.sum())
    pts = d[hit] * t[:, None]
    pts[:, 2] += sensor_z
    g = is_ground[hit]
    pts[g, 2] += rng.normal(0, 0.02, g.sum())
    pts = pts.astype(dtype)
    pts = _settle_segments(pts, dtype)
    out = np.empty((pts.shape[0], 5), dtype)
    out[:, :3] = pts
    out[:, 3] = rng.uniform(0, 1, pts.shape[0])
    out[:, 4] = rng.uniform(0, 1, pts.shape[0])
    return out


def outline_segment(angle32, dtype):
    """seg = int32(floor((atan2 + pi) / (2 pi / 150))) in `dtype` arithmetic from a float32 atan2 value (the reference's
    Processor.project_5D under numpy's per-op rounding; float16 ops compute in float32 and round)."""
    dtype = np.dtype(dtype)
    a = np.asarray(angle32, np.float32).astype(dtype)
    pi_t, step_t = dtype.type(np.pi), dtype.type(2 * np.pi / 150)
    if dtype == np.float16:
        s = (a.astype(np.float32) + np.float32(pi_t)).astype(np.float16)
        q = (s.astype(np.float32) / np.float32(step_t)).astype(np.float16)
    else:
        q = (a + pi_t) / step_t
    return np.floor(q).astype(np.int32)


def _settle_segments(pts, dtype, ulps=2):
    moved = 0
    for _ in range(64):
        x, y = pts[:, 0].astype(np.float32), pts[:, 1].astype(np.float32)
        a = np.arctan2(y, x)
        segs = [outline_segment(a, dtype)]
        lo = hi = a
        for _k in range(ulps):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            segs += [outline_segment(lo, dtype), outline_segment(hi, dtype)]
        bad = np.zeros(len(pts), bool)
        for sg in segs[1:]:
            bad |= sg != segs[0]
        if not bad.any():
            break
        moved += int(bad.sum())
        rot = 2e-3
        xb, yb = pts[bad, 0].astype(np.float64), pts[bad, 1].astype(np.float64)
        pts[bad, 0] = (np.cos(rot) * xb - np.sin(rot) * yb).astype(dtype)
        pts[bad, 1] = (np.sin(rot) * xb + np.cos(rot) * yb).astype(dtype)
    else:
        raise RuntimeError("outline_scene: could not settle segment indices")
    _settle_segments.last_moved = moved
    return pts


# ---- PP-score sequence (cpd_amd.ppscore) ---------------------------------------------------------------------------------

def ppscore_sequence(seed, n_frames, n_az, dtype=np.float16, origin=(0.0, 0.0, 0.0), n_parked=12, n_moving=10, frame_step=1):
    """A short drive for the PP-score precompute (cpd_amd.ppscore): `n_frames` sweeps of the waymo_cloud beam pattern (64
    beams x n_az azimuths, sensor 2 m above z = 0, 75 m range, 2 cm range noise), each ray-cast from an ego pose that moves
    0.35 m and yaws 0.4 deg per frame, against
      * a static world: flat ground, the waymo_cloud ring of 12 buildings, `n_parked` parked vehicle-size boxes;
      * `n_moving` boxes at constant velocity (0.3..1.2 m per frame along their heading), which leave points where the other
        traversals see nothing.
    Returns (frames, poses): frames[k] is [N_k, 5] of `dtype` (x, y, z, intensity, elongation in the vehicle frame, as Waymo
    frames are saved), poses[k] the float64 4x4 vehicle -> world matrix with `origin` added to its translation (Waymo
    translations are thousands of metres: that is where the float32 rounding in world coordinates shows). frame_step = 5
    returns every fifth sweep of the drive (the traversals of the default window) without casting the ones between."""
    dtype = np.dtype(dtype)
    if dtype not in (np.float16, np.float32):
        raise TypeError("ppscore_sequence: float16 or float32")
    rng = np.random.default_rng(seed + 9000)
    sensor_z = 2.0
    elev = np.deg2rad(np.linspace(-17.6, 2.4, 64))
    az = np.linspace(0.0, 2 * np.pi, n_az, endpoint=False)
    e, a = np.meshgrid(elev, az, indexing="ij")
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], -1).reshape(-1, 3)
    dz = d[:, 2]
    t_ground = np.where(dz < -1e-6, -sensor_z / np.minimum(dz, -1e-6), np.inf)
    static, moving = [], []
    for k in range(12):
        ang = 2 * np.pi * k / 12
        size = (rng.uniform(8, 14), rng.uniform(8, 14), rng.uniform(6, 14))
        static.append((np.array([62 * np.cos(ang), 62 * np.sin(ang), size[2] / 2]), size, ang))
    for _ in range(n_parked):
        r, ang = rng.uniform(6, 40), rng.uniform(0, 2 * np.pi)
        size = (rng.uniform(3.6, 5.2), rng.uniform(1.7, 2.2), rng.uniform(1.4, 2.1))
        static.append((np.array([r * np.cos(ang), r * np.sin(ang), size[2] / 2]), size, rng.uniform(-np.pi, np.pi)))
    for _ in range(n_moving):
        r, ang = rng.uniform(6, 30), rng.uniform(0, 2 * np.pi)
        size = (rng.uniform(3.6, 5.2), rng.uniform(1.7, 2.2), rng.uniform(1.4, 2.1))
        yaw, speed = rng.uniform(-np.pi, np.pi), rng.uniform(0.3, 1.2)
        moving.append((np.array([r * np.cos(ang), r * np.sin(ang), size[2] / 2]), size, yaw,
                       speed * np.array([np.cos(yaw), np.sin(yaw), 0.0])))
    frames, poses = [], []
    for k in range(0, n_frames * frame_step, frame_step):
        yaw_k = np.deg2rad(0.4) * k
        ego = np.array([0.35 * k, 0.05 * np.sin(0.5 * k), 0.0])
        cs, sn = np.cos(yaw_k), np.sin(yaw_k)
        rot = np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]])
        t_best = t_ground.copy()
        for c, size, yaw in static + [(c0 + k * v, size, yaw) for c0, size, yaw, v in moving]:
            t_best = np.minimum(t_best, _ray_obb(d, sensor_z, rot.T @ (c - ego), size, yaw - yaw_k))
        hit = np.isfinite(t_best) & (t_best < 75.0)
        t = t_best[hit] + rng.normal(0, 0.02, hit.sum())
        pts = d[hit] * t[:, None]
        pts[:, 2] += sensor_z
        out = np.empty((pts.shape[0], 5), dtype)
        out[:, :3] = pts
        out[:, 3] = rng.uniform(0, 1, pts.shape[0])
        out[:, 4] = rng.uniform(0, 1, pts.shape[0])
        pose = np.eye(4)
        pose[:3, :3] = rot
        pose[:3, 3] = ego + np.asarray(origin, np.float64)
        frames.append(out)
        poses.append(pose)
    return frames, poses


# ---- C_PROTO refiner input (cpd_amd.cproto) --------------------------------------------------------------------------------

def cproto_sequence(seed, n_az=1100, dtypes=(np.float16, np.float32, np.float16)):
    """A short sequence for the C_PROTO refiner's first stage (cpd_amd.cproto): len(dtypes) outline_scene sweeps with poses
    and the info list an initial label generator would have left (`outline_box` [K, 7] float64, `outline_cls`, `outline_ids`,
    `pose`), the boxes being the scene's objects with jittered centre (N(0, 0.12 m)), size (x 0.92..1.15) and heading
    (N(0, 0.04 rad)), plus the low clutter as 'Dis_Small', which the refiner skips.
      * even frames are the sweep of scene `seed` from one pose, so an object keeps its track id and its place: ids recur
        and their prototypes are static;
      * odd frames are scene `seed + 1` from a pose 6 m on, with ids of their own -- except that its even-numbered vehicles
        take the ids of scene `seed`'s, whose global position therefore jumps by metres: the moving tracks.
    Returns (frames, infos): frames[k] is [N_k, 5] of dtypes[k]."""
    rng = np.random.default_rng(seed + 11000)
    frames, infos = [], []
    for k, dt in enumerate(dtypes):
        odd = k % 2
        pts = outline_scene(seed + odd, np.dtype(dt), n_az=n_az)
        objs = outline_scene.last_objects
        yaw_k = np.deg2rad(3.0) * odd
        pose = np.eye(4)
        pose[:3, :3] = [[np.cos(yaw_k), -np.sin(yaw_k), 0.0], [np.sin(yaw_k), np.cos(yaw_k), 0.0], [0.0, 0.0, 1.0]]
        pose[:3, 3] = [1200.0 + 6.0 * odd, -340.0 + 0.5 * odd, 12.0]
        boxes, cls, ids = [], [], []
        for j, (c, size, yaw, name) in enumerate(objs):
            sz = np.asarray(size) * rng.uniform(0.92, 1.15, 3)
            ctr = np.array([c[0], c[1], sz[2] / 2]) + np.append(rng.normal(0, 0.12, 2), 0.0)
            boxes.append([ctr[0], ctr[1], ctr[2], sz[0], sz[1], sz[2], yaw + rng.normal(0, 0.04)])
            cls.append(name)
            ids.append(10 + j if name == 'Vehicle' and j % 2 == 0 else 100 * odd + 10 + j)
        frames.append(pts)
        infos.append(dict(outline_box=np.array(boxes, np.float64), outline_cls=np.array(cls), outline_ids=np.array(ids),
                          pose=pose))
    return frames, infos
