"""cpd_kitti_fov_points and cpd_kitti_export on the device against the numpy restatement (tests/ref_kitti2waymo.py) and the reference's
golden (tests/golden/kitti2waymo.npz), and evaluate_split end to end.

The FOV kernel's decisions and rows are compared bit for bit (the kernel computes the restatement's float32 expressions op by op).
The export's keep lists, counts and labels are exact; its real values are allowed 4 x tol_<key> of the golden: the maker measures,
per key, the largest distance between the reference's output and a float64 restatement of the same formulas, and the factor covers
the device's cosf / sinf / atan2f differing from numpy's by a couple of float32 steps on top of numpy's own rounding."""
import numpy as np
import pytest
import torch

import ref_kitti2waymo as R
from cpd_amd import kitti2waymo as K
from cpd_amd import ops

pytestmark = pytest.mark.gpu

KEYS = ("boxes_lidar", "location", "dimensions", "rotation_y", "alpha", "bbox")
TILE = K.TILE
SENTINEL = 7.0


@pytest.fixture(scope="module")
def g(golden):
    return golden("kitti2waymo")


def offsets(n):
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run_fov(points, lens, records, z_shift=1.55, nfo=4):
    """one launch -> (out [n, nfo], index [n], count [B]) host arrays; rows the kernel does not write hold SENTINEL / -5"""
    start = offsets(lens)
    n = len(points)
    dev = torch.device("cuda")
    pts = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev)
    out = torch.full((n, nfo), SENTINEL, dtype=torch.float32, device=dev)
    index = torch.full((n,), -5, dtype=torch.int32, device=dev)
    _, count = ops.kitti_fov_points(pts, torch.from_numpy(start).to(dev), int(max(lens, default=0)), torch.from_numpy(np.ascontiguousarray(records, np.int32)).to(dev),
                                    z_shift, nfo, out=out, out_index=index)
    return out.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy()


def check_fov(points, lens, records, z_shift=1.55, nfo=4):
    start = offsets(lens)
    out, index, count = run_fov(points, lens, records, z_shift, nfo)
    want, want_count = R.fov_host(points, start, records, z_shift, nfo)
    kept = R.fov_kept(points, start, records)
    assert np.array_equal(count, want_count)
    for f in range(len(lens)):
        a, b, k = start[f], start[f + 1], count[f]
        assert np.array_equal(index[a:a + k], kept[f])
        assert np.array_equal(bits(out[a:a + k]), bits(want[a:a + k]))
        assert (out[a + k:b] == SENTINEL).all() and (index[a + k:b] == -5).all()         # rows beyond the count are left alone
    return out, index, count


def test_fov_golden_frames_one_launch_against_three(hip, g):
    pts, lens, rec = g["fov_points"], g["fov_n"].tolist(), g["fov_frames"]
    out, index, count = check_fov(pts, lens, rec)
    start = offsets(lens)
    for f in range(3):
        a, b = start[f], start[f + 1]
        assert np.array_equal(np.flatnonzero(g["fov_flag"][a:b]), index[a:a + count[f]])        # the reference's own decisions
        o1, i1, c1 = run_fov(pts[a:b], [b - a], rec[f:f + 1])
        assert c1[0] == count[f] and np.array_equal(bits(o1), bits(out[a:b])) and np.array_equal(i1, index[a:b])
    again = run_fov(pts, lens, rec)
    assert np.array_equal(bits(again[0]), bits(out)) and np.array_equal(again[1], index) and np.array_equal(again[2], count)


def test_fov_frame_lengths_round_the_wave_and_the_tile(hip, g):
    rng = np.random.default_rng(11)
    lens = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, 0, 257]
    pts = R.gen_points(rng, sum(lens), span=40.0)
    rec = g["fov_frames"][np.arange(len(lens)) % 3]
    _, _, count = check_fov(pts, lens, rec)
    assert count[0] == 0 and count[9] == 0 and 0 < count[8] < lens[8]


def test_fov_keeps_everything_nothing_and_an_empty_frame_between(hip, g):
    rng = np.random.default_rng(12)
    n = 2 * TILE + 100
    front = np.stack([rng.uniform(8, 40, n), rng.uniform(-1, 1, n), rng.uniform(-1.0, 0.0, n), rng.uniform(0, 1, n)], 1).astype(np.float32)
    behind = front * np.float32([-1, 1, 1, 1])
    pts = np.concatenate([front, behind, front[:300]])
    lens = [n, 0, n, 300]
    rec = g["fov_frames"][[0, 1, 1, 0]]
    _, _, count = check_fov(pts, lens, rec)
    assert count.tolist() == [n, 0, 0, 300]


@pytest.mark.parametrize("ld,nfo", [(4, 4), (4, 6), (6, 4), (6, 6), (3, 3)])
def test_fov_row_pitches(hip, g, ld, nfo):
    rng = np.random.default_rng(13)
    lens = [TILE + 37, 129]
    xyzi = R.gen_points(rng, sum(lens), span=40.0)
    pts = np.concatenate([xyzi, rng.uniform(0, 1, (len(xyzi), 2)).astype(np.float32)], 1)[:, :ld]
    out, _, count = check_fov(pts, lens, g["fov_frames"][:2], z_shift=0.25, nfo=nfo)
    assert count.min() > 0 and not out[:count[0], 3:].any()


def test_fov_exact_calibration_on_the_borders(hip, g):
    """V2C an axis permutation (rect = (-y, -z, x)), R0 the identity, P2 = [[512, 0, 608, 0], [0, 512, 184, 0], [0, 0, 1, 0]], image
    370 x 1224: u = (512 rx + 608 rz) / rz, v = (512 ry + 184 rz) / rz, depth = rz, every product and sum an exact integer."""
    rec = g["fov_frames"][2:3]
    assert R.unpack(rec[0])[2:] == (370, 1224) and R.unpack(rec[0])[1][0, 0] == 512
    cases = [((16, 19, 0), True),            # rx = -19, rz = 16: u = 0
             ((64, -77, 0), False),          # rx = 77, rz = 64: u = 1224 = w
             ((1024, -1231, 0), True),       # u = 1223.5
             ((64, 0, -23.25), False),       # ry = 23.25, rz = 64: v = 370 = h
             ((64, 0, 23), True),            # ry = -23, rz = 64: v = 0
             ((128, 0, -46.25), True),       # v = 369
             ((0, 1, 0), False),             # rect_z = depth = 0: u = -inf
             ((0, -1, 0), False),            # u = +inf
             ((0, 0, 0), False),             # 0 / 0
             ((-16, 0, 0), False),           # u = 608, v = 184, depth = -16
             ((16, 0, 0), True),             # the image centre
             ((16, 19.03125, 0), False)]     # u = -1
    pts = np.array([list(c[0]) + [0.5] for c in cases], np.float32)
    want = np.array([c[1] for c in cases])
    for rep in (1, 90):                      # alone, and tiled over a wave and a round boundary
        p = np.tile(pts, (rep, 1))
        _, index, count = check_fov(p, [len(p)], rec)
        assert count[0] == want.sum() * rep and np.array_equal(index[:count[0]], np.flatnonzero(np.tile(want, rep)))


# ---- export ---------------------------------------------------------------------------------------------------------------

def run_export(boxes, scores, labels, lens, records, mode):
    dev = torch.device("cuda")
    start = offsets(lens)
    n = len(boxes)
    buf = torch.full((21 * n + len(lens),), -9, dtype=torch.int32, device=dev)
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    got = ops.kitti_export(t(np.asarray(boxes, np.float32).reshape(-1, 7), torch.float32), t(scores, torch.float32), t(labels, torch.int32),
                           torch.from_numpy(start).to(dev), torch.from_numpy(np.ascontiguousarray(records, np.int32)).to(dev), mode, out=buf)
    return {k: v.cpu().numpy() for k, v in got.items() if k != "buffer"}, start


def close(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = float(np.abs(got - ref).max(initial=0.0))
    print("%s: max error %.3g (allowed %.3g)" % (what, err, 4 * tol))
    assert err <= 4 * tol, what


def split(got, a, k):
    return {"boxes_lidar": got["boxes_lidar"][a:a + k], "location": got["camera"][a:a + k, 0:3], "dimensions": got["camera"][a:a + k, 3:6],
            "rotation_y": got["camera"][a:a + k, 6], "alpha": got["alpha"][a:a + k], "bbox": got["bbox"][a:a + k]}


def test_export_golden_predict(hip, g):
    got, start = run_export(g["exp_boxes"], g["exp_scores"], g["exp_labels"], g["exp_n"].tolist(), g["exp_frames"], K.MODE_PREDICT)
    assert np.array_equal(got["count"], g["exp_out_n"])
    out_at = offsets(g["exp_out_n"])
    keep_at = 0
    for f, name in enumerate(g["exp_names"]):
        a, k, o = start[f], got["count"][f], out_at[f]
        keep = g["exp_keep"][keep_at:keep_at + k]
        keep_at += k
        assert np.array_equal(got["score"][a:a + k], g["exp_scores"][a:start[f + 1]][keep])        # the keep list, in order
        assert np.array_equal(got["score"][a:a + k], g["exp_out_score"][o:o + k])
        assert np.array_equal(g["classes"][got["label"][a:a + k] - 1], g["exp_out_name"][o:o + k])
        assert (got["label"][a + k:start[f + 1]] == -9).all()                                         # rows beyond the count are left alone
        mine = split(got, a, k)
        for key in KEYS if name != "straddle" else ("bbox",):
            close(mine[key], g["exp_out_" + key][o:o + k], float(g["tol_" + key]), "%s of frame %s" % (key, name))


def test_export_golden_camera(hip, g):
    boxes = g["cam_boxes"].copy()
    boxes[:, 2] += boxes[:, 5] / 2                       # merge's z += h / 2; the kernel starts at boxes3d_lidar_to_kitti_camera
    got, start = run_export(boxes, None, None, g["cam_n"].tolist(), g["cam_frames"], K.MODE_CAMERA)
    assert np.array_equal(got["count"], g["cam_n"])
    for f in range(len(g["cam_n"])):
        a, k = start[f], got["count"][f]
        mine = split(got, a, k)
        for key in KEYS:
            close(mine[key], g["cam_out_" + key][a:a + k], float(g["tol_" + key]), "camera %s of frame %d" % (key, f))


def drawn_boxes(rng, n, rec):
    """gen_boxes with every eighth box too long for the filter, redrawn until the golden's margins hold"""
    for _ in range(50):
        boxes, scores, labels = R.gen_boxes(rng, n)
        boxes[3::8, 3] = rng.uniform(5.5, 7.0, len(boxes[3::8]))
        t = R.export_frame(boxes, scores, labels, rec, R.MODE_PREDICT)
        if (np.abs(t["length"] - 5) >= 1e-3).all() and (np.abs(t["dis"]) >= 1e-3).all() and (np.abs(t["rect_z"]) >= 0.5).all():
            return boxes, scores, labels
    raise AssertionError("no draw meets the margins")


@pytest.mark.parametrize("mode", [K.MODE_PREDICT, K.MODE_CAMERA])
def test_export_segment_sizes(hip, g, mode):
    rng = np.random.default_rng(21)
    lens = [0, 1, 63, 64, 65, 257]
    rec = g["fov_frames"][np.arange(len(lens)) % 3]
    parts = [drawn_boxes(rng, n, rec[f]) for f, n in enumerate(lens)]
    boxes, scores, labels = (np.concatenate([p[i] for p in parts]) for i in range(3))
    if mode == K.MODE_CAMERA:
        boxes[:, 2] -= np.float32(1.55)
    got, start = run_export(boxes, scores, labels, lens, rec, mode)
    want = R.export_host(boxes, scores, labels, start, rec, mode)
    assert np.array_equal(got["count"], want["count"])
    assert (got["count"] == lens).all() if mode == K.MODE_CAMERA else (got["count"][2:] < lens[2:]).all()
    for f in range(len(lens)):
        a, k = start[f], got["count"][f]
        assert np.array_equal(got["label"][a:a + k], want["label"][a:a + k]) and np.array_equal(got["score"][a:a + k], want["score"][a:a + k])
        assert (got["label"][a + k:start[f + 1]] == -9).all()
        mine, ref = split(got, a, k), split(want, a, k)
        for key in KEYS:
            close(mine[key], ref[key], float(g["tol_" + key]), "%s of a segment of %d" % (key, lens[f]))


# ---- end to end -----------------------------------------------------------------------------------------------------------

KITTI_CLASSES = ["Car", "Pedestrian", "Cyclist"]


def gt_annos(rng, calib, shape):
    """two easy ground-truth boxes of every class, through the host conversions"""
    labels = np.repeat([1, 2, 3], 2)
    size = np.array([[4.2, 1.8, 1.5], [0.8, 0.7, 1.75], [1.8, 0.6, 1.7]])[labels - 1]
    x = rng.uniform(7.0, 14.0, 6)
    boxes = np.concatenate([np.stack([x, x * rng.uniform(-0.3, 0.3, 6), -1.7 + size[:, 2] / 2], 1), size, rng.uniform(-3, 3, (6, 1))], 1).astype(np.float32)
    cam = K.boxes3d_lidar_to_kitti_camera(boxes.copy(), calib)
    return {"name": np.array(KITTI_CLASSES)[labels - 1], "truncated": np.zeros(6), "occluded": np.zeros(6), "alpha": np.zeros(6),
            "bbox": K.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=shape).astype(np.float64), "dimensions": cam[:, 3:6].astype(np.float64),
            "location": cam[:, 0:3].astype(np.float64), "rotation_y": cam[:, 6].astype(np.float64)}


class Recorder:
    def __init__(self, engine):
        self.engine, self.preds, self.points = engine, [], []

    def forward(self, points):
        res = self.engine.forward(points)
        self.points += list(points)
        self.preds += [{k: v.clone() for k, v in d.items() if k in ("pred_boxes", "pred_scores", "pred_labels")} for d in res]
        return res


def test_evaluate_split_end_to_end(hip, g, tmp_path):
    """evaluate_split on a synthetic KITTI directory against the same engine's detections pushed through the injected restatement:
    annos within the golden's tolerances, the AP string equal. One rule differs from the golden's `straddle` case, where the
    clipped `bbox` IS compared: a random-weight engine puts boxes anywhere, and a corner within 0.5 m of the camera plane
    amplifies one float32 step of cosf / sinf in its depth into whole pixels, or flips the clipped edge between 0 and w - 1, so
    no tolerance derived from the golden (whose straddling corners keep 0.2 m) holds for such a row. Those rows are compared on
    every key but `bbox`; the test asserts that `bbox` rows remain."""
    from cpd_amd.engine import CenterPointEngine, ModelConfig, init_state_dict
    from cpd_amd.synthetic import waymo_cloud
    rng = np.random.default_rng(31)
    (tmp_path / "velodyne").mkdir(), (tmp_path / "calib").mkdir()
    infos, clouds, calibs = [], [], []
    for f in range(3):
        name = "%06d" % f
        pts = waymo_cloud(f, n_points=40000)[:, :4].copy()
        pts[:, :2] *= 0.3
        pts[:, 2] -= 1.55 - 0.3                                    # a KITTI sensor sits lower than the synthetic one
        pts.tofile(tmp_path / "velodyne" / (name + ".bin"))
        (tmp_path / "calib" / (name + ".txt")).write_text(R.calib_text(f))
        calib = K.Calibration(tmp_path / "calib" / (name + ".txt"))
        shape = np.array(R.IMAGE_SHAPES[f], np.int32)
        infos.append({"point_cloud": {"num_features": 4, "lidar_idx": name}, "image": {"image_idx": name, "image_shape": shape},
                      "annos": gt_annos(rng, calib, shape)})
        clouds.append(pts), calibs.append(calib)
    cfg = ModelConfig(point_cloud_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 4.0], post_center_limit_range=[-20, -20, -2, 20, 20, 4],
                      bev_num_filters=[64, 128], bev_num_upsample_filters=[128, 128], bev_layer_nums=[1, 1], max_obj_per_sample=100,
                      num_point_features=4)
    rec = Recorder(CenterPointEngine(cfg, init_state_dict(cfg, seed=1)))
    result, ret, annos = K.evaluate_split(rec, infos, tmp_path, KITTI_CLASSES, batch=2)
    assert len(annos) == 3 and sum(len(a["score"]) for a in annos) > 0, "the engine found nothing: the test compares nothing"
    # the crop the engine was fed is the restatement's
    for f in range(3):
        want, count = R.fov_host(clouds[f], offsets([len(clouds[f])]), R.frame_record(calibs[f], R.IMAGE_SHAPES[f])[None], 1.55, 4)
        assert np.array_equal(bits(rec.points[f].cpu().numpy()), bits(want[:count[0]])) and 0 < count[0] < len(clouds[f])
    # the same detections through the injected restatement
    host_preds = [{k: v.cpu() for k, v in d.items()} for d in rec.preds]
    batch = {"frame_id": [i["point_cloud"]["lidar_idx"] for i in infos], "calib": calibs, "image_shape": [i["image"]["image_shape"] for i in infos]}
    want = K.generate_prediction_dicts(batch, host_preds, KITTI_CLASSES, _export=R.export_host)
    bbox_rows = 0
    for f, (a, w) in enumerate(zip(annos, want)):
        assert list(a.keys()) == list(w.keys()) and a["frame_id"] == w["frame_id"]
        assert np.array_equal(a["name"], w["name"]) and np.array_equal(a["score"], w["score"])
        if not len(a["score"]):
            continue
        t = R.export_frame(host_preds[f]["pred_boxes"].numpy(), host_preds[f]["pred_scores"].numpy(), host_preds[f]["pred_labels"].numpy(),
                           R.frame_record(calibs[f], R.IMAGE_SHAPES[f]), R.MODE_PREDICT)
        clear = (np.abs(t["rect_z"]) >= 0.5).all(1)               # the golden's condition: no corner within 0.5 m of the camera plane
        bbox_rows += int(clear.sum())
        for key in KEYS:
            rows = clear if key == "bbox" else np.ones(len(clear), bool)
            close(a[key][rows], w[key][rows], float(g["tol_" + key]), "%s of frame %d" % (key, f))
    assert bbox_rows > 0, "no bbox row was compared"
    print("bbox rows compared: %d of %d" % (bbox_rows, sum(len(a["score"]) for a in annos)))
    result_host, ret_host = K.evaluation(want, [i["annos"] for i in infos], KITTI_CLASSES)
    assert isinstance(result, str) and result == result_host and ret == ret_host
