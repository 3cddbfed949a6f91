"""numpy restatement of the two device stages of cpd_amd.kitti2waymo (csrc/kitti2waymo.hip), with the signatures of its `_fov=` /
`_export=` hooks, plus the input generators the golden maker and the GPU tests share.

Point stage: float32, products and sums one at a time from left to right (numpy's element-wise operations do not fuse), which is
what the kernel computes; the reference's own matrix products may associate or fuse differently, which is why the golden maker
sets a band round the image borders aside. Export: the reference's dtypes under numpy >= 2 (`ft=np.float32`), or every float
operation in float64 (`ft=np.float64`): the distance between the two is the measure of the test's tolerances."""
import numpy as np

FRAME_WORDS = 26
MODE_PREDICT, MODE_CAMERA = 0, 1
CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]

# two real-shaped KITTI calibrations (P2, R0_rect, Tr_velo_to_cam) and an exact one: an axis permutation, identity R0, integer P2
CALIB_LINES = [
    {"P2": "7.215377e+02 0.000000e+00 6.095593e+02 4.485728e+01 0.000000e+00 7.215377e+02 1.728540e+02 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03",
     "R0_rect": "9.999239e-01 9.837760e-03 -7.445048e-03 -9.869795e-03 9.999421e-01 -4.278459e-03 7.402527e-03 4.351614e-03 9.999631e-01",
     "Tr_velo_to_cam": "7.533745e-03 -9.999714e-01 -6.166020e-04 -4.069766e-03 1.480249e-02 7.280733e-04 -9.998902e-01 -7.631618e-02 9.998621e-01 7.523790e-03 1.480755e-02 -2.717806e-01"},
    {"P2": "7.070493e+02 0.000000e+00 6.040814e+02 4.575831e+01 0.000000e+00 7.070493e+02 1.805066e+02 -3.454157e-01 0.000000e+00 0.000000e+00 1.000000e+00 4.981016e-03",
     "R0_rect": "9.999128e-01 1.009263e-02 -8.511932e-03 -1.012729e-02 9.999406e-01 -4.037671e-03 8.470675e-03 4.123522e-03 9.999556e-01",
     "Tr_velo_to_cam": "6.927964e-03 -9.999722e-01 -2.757829e-03 -2.457729e-02 -1.162982e-03 2.749836e-03 -9.999955e-01 -6.127237e-02 9.999753e-01 6.931141e-03 -1.143899e-03 -3.321029e-01"},
    {"P2": "512 0 608 0 0 512 184 0 0 0 1 0", "R0_rect": "1 0 0 0 1 0 0 0 1", "Tr_velo_to_cam": "0 -1 0 0 0 0 -1 0 1 0 0 0"},
]
IMAGE_SHAPES = [(375, 1242), (370, 1224), (370, 1224)]


def calib_text(i, r0=True):
    """a KITTI calib file of calibration i (P0 / P1 / P3 / Tr_imu_to_velo lines filled with P2's or zeros, as a real file has seven lines)"""
    c = CALIB_LINES[i]
    lines = ["P0: " + c["P2"], "P1: " + c["P2"], "P2: " + c["P2"], "P3: " + c["P2"]]
    if r0:
        lines.append("R0_rect: " + c["R0_rect"])
    lines += ["Tr_velo_to_cam: " + c["Tr_velo_to_cam"], "Tr_imu_to_velo: " + " ".join(["0"] * 12)]
    return "\n".join(lines) + "\n"


def calib_dict(i):
    c = CALIB_LINES[i]
    arr = lambda s, shape: np.array(s.split(" "), np.float32).reshape(shape)
    return {"P2": arr(c["P2"], (3, 4)), "P3": arr(c["P2"], (3, 4)), "R0": arr(c["R0_rect"], (3, 3)), "Tr_velo2cam": arr(c["Tr_velo_to_cam"], (3, 4))}


def frame_record(calib, shape):
    """int32 [FRAME_WORDS] of an object with V2C / R0 / P2 (any Calibration): the layout of include/cpd_hip.h"""
    rec = np.zeros(FRAME_WORDS, np.int32)
    rec[0:12] = np.ascontiguousarray(np.dot(calib.V2C.T, calib.R0.T), np.float32).reshape(-1).view(np.int32)
    rec[12:24] = np.ascontiguousarray(calib.P2, np.float32).reshape(-1).view(np.int32)
    rec[24], rec[25] = int(shape[0]), int(shape[1])
    return rec


def unpack(rec, ft=np.float32):
    rec = np.ascontiguousarray(rec, np.int32)
    return rec[0:12].view(np.float32).reshape(4, 3).astype(ft), rec[12:24].view(np.float32).reshape(3, 4).astype(ft), int(rec[24]), int(rec[25])


def lidar_to_rect(m, x, y, z):
    return tuple(((x * m[0, j] + y * m[1, j]) + z * m[2, j]) + m[3, j] for j in range(3))


def rect_to_img(p, rx, ry, rz):
    with np.errstate(all="ignore"):
        h = [((rx * p[i, 0] + ry * p[i, 1]) + rz * p[i, 2]) + p[i, 3] for i in range(3)]
        return h[0] / rz, h[1] / rz, h[2] - p[2, 3]


def fov_uvd(xyz, rec, ft=np.float32):
    m, p, h, w = unpack(rec, ft)
    xyz = np.asarray(xyz).astype(ft)
    with np.errstate(all="ignore"):
        return rect_to_img(p, *lidar_to_rect(m, xyz[:, 0], xyz[:, 1], xyz[:, 2]))


def fov_flag(xyz, rec, ft=np.float32):
    _, _, h, w = unpack(rec)
    u, v, d = fov_uvd(xyz, rec, ft)
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (u < ft(w)) & (v >= 0) & (v < ft(h)) & (d >= 0)


def fov_host(points, frame_start, frames, z_shift, n_feat_out):
    """the `_fov=` hook: -> (out [n, n_feat_out] float32, frame f's kept rows from row frame_start[f]; counts [B] int32)"""
    points = np.asarray(points, np.float32)
    out = np.zeros((len(points), n_feat_out), np.float32)
    count = np.zeros(len(frame_start) - 1, np.int32)
    for f in range(len(count)):
        a, b = int(frame_start[f]), int(frame_start[f + 1])
        keep = np.flatnonzero(fov_flag(points[a:b, :3], frames[f]))
        count[f] = len(keep)
        rows = points[a:b][keep]
        out[a:a + len(keep), 0:2] = rows[:, 0:2]
        out[a:a + len(keep), 2] = (rows[:, 2].astype(np.float64) + z_shift).astype(np.float32)
    return out, count


def fov_kept(points, frame_start, frames):
    """per frame the in-frame indices of the kept points"""
    return [np.flatnonzero(fov_flag(np.asarray(points, np.float32)[int(a):int(b), :3], frames[f])).astype(np.int32)
            for f, (a, b) in enumerate(zip(frame_start[:-1], frame_start[1:]))]


def export_frame(boxes, scores, labels, rec, mode, ft=np.float32):
    """One frame. -> dict: keep (input rows kept, in order), boxes_lidar [k, 7], score, label, camera [k, 7], alpha, bbox [k, 4], and
    the margins the golden maker asserts: length (l after the shrink, all input rows), dis (dis1 - dis2 of the kept label-1 rows),
    rect_z [k, 8] of the corners."""
    m, p, h, w = unpack(rec, ft)
    b = np.asarray(boxes, np.float32).reshape(-1, 7).astype(ft)
    n = len(b)
    scores = np.zeros(n, np.float32) if scores is None else np.asarray(scores, np.float32)
    labels = np.zeros(n, np.int32) if labels is None else np.asarray(labels).astype(np.int32)
    x, y, z, l, wd, hh, r = (b[:, i].copy() for i in range(7))
    keep = np.ones(n, bool)
    length = l.copy()
    dis = np.zeros(0)
    with np.errstate(all="ignore"):
        if mode == MODE_PREDICT:
            z = z - ft(1.55)
            nz = labels != 0
            if nz.any():
                z = np.where(nz, z + ft(0.1), z)
                l = np.where(nz, l - ft(0.2), l)
                wd = np.where(nz, wd - ft(0.2), wd)
                hh = np.where(nz, hh - ft(0.1), hh)
                keep = l < ft(5)
            length = l.copy()
            x, y, z, l, wd, hh, r, scores, labels = (a[keep] for a in (x, y, z, l, wd, hh, r, scores, labels))
            one = labels == 1
            cs, sn = np.cos(r), np.sin(r)
            dis0 = np.sqrt((x * x + y * y) + z * z)
            new_d = ft(0.1) + (dis0 / ft(60)) * ft(0.4 - 0.1)
            half = np.where(dis0 > ft(60), (0.1 + 1.0 * (0.4 - 0.1)) / 2, (new_d / ft(2)).astype(np.float64))
            c64, s64, x64, y64, z64 = (a.astype(np.float64) for a in (cs, sn, x, y, z))
            x1, y1, x2, y2 = half * c64 + x64, half * s64 + y64, -half * c64 + x64, -half * s64 + y64
            dis1 = np.sqrt(((x1 * x1 + y1 * y1) + z64 * z64) + 1.0)
            dis2 = np.sqrt(((x2 * x2 + y2 * y2) + z64 * z64) + 1.0)
            first = dis1 < dis2
            x = np.where(one, np.where(first, x1, x2).astype(ft), x)
            y = np.where(one, np.where(first, y1, y2).astype(ft), y)
            dis = (dis1 - dis2)[one]
        z = z - hh / ft(2)
        cx, cy, cz = lidar_to_rect(m, x, y, z)
        ry = -r - ft(np.pi / 2)
        cr, sr = np.cos(ry), np.sin(ry)
        hl, hw = l / ft(2), wd / ft(2)
        zero, one_ = ft(0), ft(1)
        us, vs, zs = [], [], []
        for k in range(8):
            xc = -hl if (k >> 1) & 1 else hl
            zc = -hw if ((k + 1) >> 1) & 1 else hw
            yc = -hh if k >= 4 else np.zeros_like(hh)
            px = cx + ((xc * cr + yc * zero) + zc * sr)
            py = cy + ((xc * zero + yc * one_) + zc * zero)
            pz = cz + ((xc * -sr + yc * zero) + zc * cr)
            u, v, _ = rect_to_img(p, px, py, pz)
            us.append(u), vs.append(v), zs.append(pz)
        us, vs = np.stack(us, 1).reshape(-1, 8), np.stack(vs, 1).reshape(-1, 8)
        bbox = np.stack([np.clip(us.min(1), 0, w - 1), np.clip(vs.min(1), 0, h - 1), np.clip(us.max(1), 0, w - 1),
                         np.clip(vs.max(1), 0, h - 1)], 1).astype(ft)
        alpha = -np.arctan2(-y, x) + ry
    return {"keep": np.flatnonzero(keep), "boxes_lidar": np.stack([x, y, z, l, wd, hh, r], 1), "score": scores, "label": labels,
            "camera": np.stack([cx, cy, cz, l, hh, wd, ry], 1), "alpha": alpha, "bbox": bbox.reshape(-1, 4), "length": length, "dis": dis,
            "rect_z": np.stack(zs, 1).reshape(-1, 8)}


def export_host(boxes, scores, labels, seg_start, frames, mode, ft=np.float32):
    """the `_export=` hook: -> dict of arrays over all n rows, frame f's kept rows from row seg_start[f], and count [B]"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 7)
    n, nb = len(boxes), len(seg_start) - 1
    out = {"boxes_lidar": np.zeros((n, 7), ft), "score": np.zeros(n, np.float32), "label": np.zeros(n, np.int32),
           "camera": np.zeros((n, 7), ft), "alpha": np.zeros(n, ft), "bbox": np.zeros((n, 4), ft), "count": np.zeros(nb, np.int32)}
    for f in range(nb):
        a, b = int(seg_start[f]), int(seg_start[f + 1])
        got = export_frame(boxes[a:b], None if scores is None else scores[a:b], None if labels is None else labels[a:b], frames[f], mode, ft)
        k = len(got["keep"])
        out["count"][f] = k
        for key in ("boxes_lidar", "score", "label", "camera", "alpha", "bbox"):
            out[key][a:a + k] = got[key]
    return out


# ---- generators -----------------------------------------------------------------------------------------------------------

def gen_points(rng, n, span=70.0):
    """[n, 4] float32 all round the sensor, on a 1 / 1024 m lattice like a real scan's millimetres; intensity in hundredths"""
    r = span * np.sqrt(rng.uniform(0.002, 1.0, n))
    a = rng.uniform(-np.pi, np.pi, n)
    pts = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.5, 1.5, n), np.round(rng.uniform(0, 1, n), 2)], 1)
    pts[:, :3] = np.round(pts[:, :3] * 1024) / 1024
    return pts.astype(np.float32)


def gen_boxes(rng, n, lift=1.55):
    """n detections in the sensor-height frame in front of the camera: (boxes [n, 7], scores [n] descending, labels [n] in 1..3)"""
    labels = rng.integers(1, 4, n).astype(np.int64)
    size = np.array([[4.4, 1.9, 1.6], [0.9, 0.8, 1.75], [1.8, 0.7, 1.7]])[labels - 1] * rng.uniform(0.85, 1.15, (n, 3))
    x = rng.uniform(6.0, 58.0, n)
    y = x * rng.uniform(-0.6, 0.6, n)
    z = -1.7 + size[:, 2] / 2 + rng.uniform(-0.2, 0.2, n) + lift
    boxes = np.concatenate([np.stack([x, y, z], 1), size, rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)
    scores = np.sort(rng.uniform(0.1, 0.95, n))[::-1].astype(np.float32)
    return boxes, scores, labels
