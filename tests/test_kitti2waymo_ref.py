"""CPU checks of the KITTI transfer-evaluation path: the numpy restatement (tests/ref_kitti2waymo.py) against the reference's golden
(tests/golden/kitti2waymo.npz, make_golden_kitti2waymo.py), and the host logic of cpd_amd.kitti2waymo with the restatement injected
for the two kernels. Tolerances of the export's real values: 4 x the golden's tol_<key> (reference against a float64 restatement),
see the maker's docstring."""
import inspect
import os

import numpy as np
import pytest
import torch

import ref_kitti2waymo as R
from cpd_amd import kitti2waymo as K

KEYS = ("boxes_lidar", "location", "dimensions", "rotation_y", "alpha", "bbox")
ANNO_KEYS = ["name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score", "boxes_lidar", "frame_id"]


@pytest.fixture(scope="module")
def g(golden):
    return golden("kitti2waymo")


def offsets(n):
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


def calib_of(g, i):
    return K.Calibration({"P2": g["calib%d_P2" % i], "R0": g["calib%d_R0" % i], "Tr_velo2cam": g["calib%d_V2C" % i]})


def which_calib(g, records):
    return [int(np.flatnonzero((g["fov_frames"] == r).all(1))[0]) for r in records]


def close(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = float(np.abs(got - ref).max(initial=0.0))
    print("%s: max error %.3g (allowed %.3g)" % (what, err, 4 * tol))
    assert err <= 4 * tol, what


def ref_annos(g):
    """the golden's reference annos, frame by frame"""
    at = offsets(g["exp_out_n"])
    out = []
    for f in range(len(g["exp_n"])):
        a, b = at[f], at[f + 1]
        out.append({k: g["exp_out_" + k][a:b] for k in ("name", "score", "truncated", "occluded") + KEYS})
    return out


def check_annos(g, annos, skip_values=()):
    ref = ref_annos(g)
    for f, (got, want) in enumerate(zip(annos, ref)):
        assert list(got.keys()) == ANNO_KEYS
        if len(want["score"]) == 0:
            for k in ANNO_KEYS[:-1]:
                assert got[k].dtype == np.float64 and not got[k].any()
            assert got["bbox"].shape == (0, 4) and got["boxes_lidar"].shape == (0, 7) and got["dimensions"].shape == (0, 3) and got["name"].shape == (0,)
            continue
        assert np.array_equal(got["name"], want["name"]) and np.array_equal(got["score"], want["score"])
        for k in ("truncated", "occluded"):
            assert got[k].dtype == np.float64 and got[k].shape == want[k].shape and not got[k].any()
        for k in KEYS:
            assert got[k].dtype == want[k].dtype == np.float32 and got[k].shape == want[k].shape
            if g["exp_names"][f] != "straddle" or k == "bbox":
                close(got[k], want[k], float(g["tol_" + k]), "%s of frame %s" % (k, g["exp_names"][f]))


def test_golden_is_data_of_the_documented_shape(g):
    assert str(g["numpy_version"]).startswith("2.")
    assert g["fov_points"].shape == (int(g["fov_n"].sum()), 4) and g["fov_frames"].shape == (3, R.FRAME_WORDS)
    assert g["fov_band"].mean() <= 1e-3
    assert list(g["exp_names"]) == ["main", "second", "emptied", "none", "exact", "straddle"]
    assert g["exp_out_n"][2] == 0 and g["exp_n"][2] > 0 and g["exp_n"][3] == 0
    assert set(g["exp_labels"].tolist()) == {1, 2, 3}
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "kitti2waymo.npz")) < 300 * 1024


def test_fov_restatement_against_the_reference(g):
    pts, start = g["fov_points"], offsets(g["fov_n"])
    flag, band = g["fov_flag"], g["fov_band"]
    kept = R.fov_kept(pts, start, g["fov_frames"])
    out, count = R.fov_host(pts, start, g["fov_frames"], 1.55, 4)
    z_at = 0
    for f in range(3):
        a, b = start[f], start[f + 1]
        mine = np.zeros(b - a, bool)
        mine[kept[f]] = True
        assert np.array_equal(mine[~band[a:b]], flag[a:b][~band[a:b]])
        assert np.array_equal(mine, flag[a:b])                    # (the maker drew inputs for which this holds inside the band too)
        assert count[f] == flag[a:b].sum()
        rows = out[a:a + count[f]]
        want = pts[a:b][flag[a:b]]
        assert np.array_equal(rows[:, :2], want[:, :2]) and not rows[:, 3:].any()
        z64 = g["fov_out_z"][z_at:z_at + count[f]]
        assert np.array_equal(rows[:, 2], z64.astype(np.float32))       # the float64 sum, rounded once
        z_at += count[f]
        assert not out[a + count[f]:b].any()
    assert z_at == len(g["fov_out_z"])
    float64_flags = np.concatenate([R.fov_flag(pts[start[f]:start[f + 1], :3], g["fov_frames"][f], np.float64) for f in range(3)])
    assert np.array_equal(float64_flags[~band], flag[~band])


def test_export_restatement_against_the_reference(g):
    start = offsets(g["exp_n"])
    got = R.export_host(g["exp_boxes"], g["exp_scores"], g["exp_labels"], start, g["exp_frames"], R.MODE_PREDICT)
    assert np.array_equal(got["count"], g["exp_out_n"])
    keep = np.concatenate([R.export_frame(g["exp_boxes"][a:b], g["exp_scores"][a:b], g["exp_labels"][a:b], g["exp_frames"][f], R.MODE_PREDICT)["keep"]
                           for f, (a, b) in enumerate(zip(start[:-1], start[1:]))])
    assert np.array_equal(keep, g["exp_keep"])
    ref = ref_annos(g)
    for f in range(len(g["exp_n"])):
        a, k = start[f], got["count"][f]
        assert np.array_equal(np.array(R.CLASSES)[got["label"][a:a + k] - 1], ref[f]["name"]) if k else True
        assert np.array_equal(got["score"][a:a + k], ref[f]["score"])
        if g["exp_names"][f] == "straddle":
            close(got["bbox"][a:a + k], ref[f]["bbox"], float(g["tol_bbox"]), "straddle bbox")
            continue
        for key, val in (("boxes_lidar", got["boxes_lidar"]), ("location", got["camera"][:, 0:3]), ("dimensions", got["camera"][:, 3:6]),
                         ("rotation_y", got["camera"][:, 6]), ("alpha", got["alpha"]), ("bbox", got["bbox"])):
            close(val[a:a + k], ref[f][key], float(g["tol_" + key]), "%s of frame %s" % (key, g["exp_names"][f]))
    # the exact tie takes the second, negative, candidate: x = -new_d / 2
    main = R.export_frame(g["exp_boxes"][:start[1]], g["exp_scores"][:start[1]], g["exp_labels"][:start[1]], g["exp_frames"][0], R.MODE_PREDICT)
    tie = np.flatnonzero((g["exp_boxes"][:start[1], 0] == 0) & (g["exp_boxes"][:start[1], 6] == 0))
    assert len(tie) == 1
    row = int(np.flatnonzero(main["keep"] == tie[0])[0])
    assert -0.2 < main["boxes_lidar"][row, 0] < -0.05 and ref[0]["boxes_lidar"][row, 0] == main["boxes_lidar"][row, 0]


@pytest.mark.parametrize("name", ["calib0", "calib1", "calib2", "calibN"])
def test_calibration_parsing_and_host_methods(g, tmp_path, name):
    path = tmp_path / "000007.txt"
    path.write_text(str(g[name + "_text"]))
    assert ("R0_rect" in str(g[name + "_text"])) == (name != "calibN")
    for c in (K.Calibration(path), K.Calibration(str(path)), K.Calibration(K.get_calib_from_file(path))):
        for attr, key in (("P2", "_P2"), ("R0", "_R0"), ("V2C", "_V2C")):
            assert getattr(c, attr).dtype == g[name + key].dtype and np.array_equal(getattr(c, attr), g[name + key])
        assert c.R0.dtype == (np.float64 if name == "calibN" else np.float32)
        assert (c.cu, c.cv, c.fu, c.fv) == (c.P2[0, 2], c.P2[1, 2], c.P2[0, 0], c.P2[1, 1])
        assert c.tx == c.P2[0, 3] / (-c.fu) and c.ty == c.P2[1, 3] / (-c.fv)
        probe = g["probe_xyz"]
        rect = c.lidar_to_rect(probe)
        assert rect.dtype == g[name + "_rect"].dtype
        np.testing.assert_allclose(rect, g[name + "_rect"], rtol=1e-6, atol=1e-5)
        img, depth = c.rect_to_img(probe + np.float32([0, 0, 45]))
        np.testing.assert_allclose(img, g[name + "_img"], rtol=1e-6, atol=1e-4)
        np.testing.assert_allclose(depth, g[name + "_depth"], rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(c.rect_to_lidar(probe), g[name + "_lidar"], rtol=1e-5, atol=1e-4)
        img2, depth2 = c.lidar_to_img(probe)
        assert np.array_equal(img2, c.rect_to_img(rect)[0]) and np.array_equal(depth2, c.rect_to_img(rect)[1])
    rec = K.frame_words([c], [(375, 1242)])
    assert rec.shape == (1, K.FRAME_WORDS) and np.array_equal(rec[0], R.frame_record(c, (375, 1242)))


def test_host_box_conversions(g):
    c = calib_of(g, 0)
    n = int(g["cam_n"][0])
    boxes = g["cam_boxes"][:n].copy()
    boxes[:, 2] += boxes[:, 5] / 2
    before = boxes.copy()
    cam = K.boxes3d_lidar_to_kitti_camera(boxes, c)
    assert np.array_equal(boxes[:, 2], before[:, 2] - before[:, 5] / 2)           # in place, as the reference
    close(cam[:, 0:3], g["cam_out_location"][:n], float(g["tol_location"]), "host location")
    assert np.array_equal(cam[:, 3:6], g["cam_out_dimensions"][:n]) and np.array_equal(cam[:, 6], g["cam_out_rotation_y"][:n])
    img = K.boxes3d_kitti_camera_to_imageboxes(cam, c, image_shape=np.array([375, 1242], np.int32))
    close(img, g["cam_out_bbox"][:n], float(g["tol_bbox"]), "host bbox")
    back = K.boxes3d_kitti_camera_to_lidar(cam, c)
    np.testing.assert_allclose(back[:, :6], before[:, :6], atol=2e-4)
    np.testing.assert_allclose(np.cos(back[:, 6]), np.cos(before[:, 6]), atol=1e-5)
    pts = g["fov_points"][:int(g["fov_n"][0])]
    flag = K.get_fov_flag(c.lidar_to_rect(pts[:, 0:3]), (375, 1242), c)
    assert np.array_equal(flag, g["fov_flag"][:len(pts)])
    boxes2d, corners = c.corners3d_to_img_boxes(K.boxes3d_to_corners3d_kitti_camera(cam))
    assert boxes2d.shape == (n, 4) and corners.shape == (n, 8, 2)


def pred_dicts_of(g, dtype=torch.int64):
    start = offsets(g["exp_n"])
    return [{"pred_boxes": torch.from_numpy(g["exp_boxes"][a:b].copy()), "pred_scores": torch.from_numpy(g["exp_scores"][a:b].copy()),
             "pred_labels": torch.from_numpy(g["exp_labels"][a:b].copy()).to(dtype)} for a, b in zip(start[:-1], start[1:])]


def batch_of(g):
    idx = which_calib(g, g["exp_frames"])
    return {"frame_id": ["%06d" % i for i in range(len(idx))], "calib": [calib_of(g, i) for i in idx],
            "image_shape": [np.array(R.IMAGE_SHAPES[i], np.int32) for i in idx]}


def test_fov_points_host_logic(g):
    start = offsets(g["fov_n"])
    clouds = [g["fov_points"][a:b] for a, b in zip(start[:-1], start[1:])]
    calibs = [calib_of(g, i) for i in range(3)]
    calls = []

    def fov(points, frame_start, frames, z_shift, n_feat_out):
        calls.append((frame_start.copy(), z_shift, n_feat_out))
        assert np.array_equal(frames, g["fov_frames"]) and np.array_equal(points, g["fov_points"])
        return R.fov_host(points, frame_start, frames, z_shift, n_feat_out)

    for mixed in (False, True):
        src = [torch.from_numpy(c.copy()) for c in clouds] if mixed else clouds
        got = K.fov_points(src, calibs, R.IMAGE_SHAPES, _fov=fov)
        assert len(got) == 3
        for f, t in enumerate(got):
            a, b = start[f], start[f + 1]
            want = g["fov_points"][a:b][g["fov_flag"][a:b]]
            assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == (len(want), 4)
            assert np.array_equal(t.numpy()[:, :2], want[:, :2]) and not t.numpy()[:, 3].any()
    assert len(calls) == 2 and np.array_equal(calls[0][0], start) and calls[0][1:] == (1.55, 4)
    assert K.fov_points([], [], []) == []
    six = K.fov_points(clouds[:1], calibs[:1], R.IMAGE_SHAPES[:1], z_shift=0.0, num_features=6, _fov=R.fov_host)[0]
    assert six.shape[1] == 6 and np.array_equal(six.numpy()[:, 2], clouds[0][g["fov_flag"][:start[1]], 2])


def test_generate_prediction_dicts_host_logic(g, tmp_path):
    pred = pred_dicts_of(g)
    before = [{k: v.clone() for k, v in d.items()} for d in pred]
    annos = K.generate_prediction_dicts(batch_of(g), pred, R.CLASSES, output_path=tmp_path, _export=R.export_host)
    for d, b in zip(pred, before):
        assert all(torch.equal(d[k], b[k]) for k in d)                 # the caller's tensors are not written
    assert [a["frame_id"] for a in annos] == ["%06d" % i for i in range(6)]
    check_annos(g, annos)
    for f, a in enumerate(annos):
        lines = (tmp_path / ("%06d.txt" % f)).read_text().splitlines()
        assert len(lines) == len(a["score"])
        assert all(ln.split(" ")[0] == a["name"][i] and len(ln.split(" ")) == 16 for i, ln in enumerate(lines))
        K.write_kitti_txt(tmp_path / "again.txt", a)                     # the call path hands the writer what it returns
        assert (tmp_path / ("%06d.txt" % f)).read_text() == (tmp_path / "again.txt").read_text()
        for i, ln in enumerate(lines):                                   # and every field sits where the KITTI format has it
            v = [float(x) for x in ln.split(" ")[3:]]
            want = [a["alpha"][i], *a["bbox"][i], a["dimensions"][i][1], a["dimensions"][i][2], a["dimensions"][i][0], *a["location"][i],
                    a["rotation_y"][i], a["score"][i]]
            assert np.abs(np.array(v) - np.array(want, np.float64)).max() <= 5.1e-5
    wide = pred_dicts_of(g)
    wide[0]["pred_boxes"] = torch.cat([wide[0]["pred_boxes"], wide[0]["pred_boxes"][:, :1]], 1)
    with pytest.raises(ValueError):
        K.generate_prediction_dicts(batch_of(g), wide, R.CLASSES, _export=R.export_host)
    assert K.generate_prediction_dicts(batch_of(g), [], R.CLASSES, _export=R.export_host) == []
    again = K.generate_prediction_dicts(batch_of(g), pred_dicts_of(g, torch.int32), R.CLASSES, _export=R.export_host)
    assert all(np.array_equal(x["bbox"], y["bbox"]) and np.array_equal(x["name"], y["name"]) for x, y in zip(annos, again))


def test_txt_writer_character_for_character(g, tmp_path):
    """the reference's annos through write_kitti_txt against the files the reference's own writer left"""
    for f, anno in enumerate(ref_annos(g)):
        path = tmp_path / ("%d.txt" % f)
        K.write_kitti_txt(path, anno)
        assert path.read_text() == str(g["exp_txt"][f])
    assert str(g["exp_txt"][0]).count("\n") == g["exp_out_n"][0] and str(g["exp_txt"][3]) == ""


def test_camera_keys_host_logic(g):
    start = offsets(g["cam_n"])
    idx = which_calib(g, g["cam_frames"])
    infos = [{"name": np.array(["Vehicle"] * (b - a)), "score": np.linspace(0.9, 0.1, b - a).astype(np.float32),
              "boxes_lidar": g["cam_boxes"][a:b].copy(), "frame_id": "%06d" % f, "alpha": np.zeros(b - a)} for f, (a, b) in enumerate(zip(start[:-1], start[1:]))]
    infos.append({"name": np.zeros(0), "score": np.zeros(0), "boxes_lidar": np.zeros((0, 7)), "frame_id": "000003"})
    keep = [i["boxes_lidar"].copy() for i in infos]
    out = K.camera_keys(infos, [calib_of(g, i) for i in idx] + [calib_of(g, 0)], [R.IMAGE_SHAPES[i] for i in idx] + [R.IMAGE_SHAPES[0]],
                        _export=R.export_host)
    assert all(np.array_equal(i["boxes_lidar"], k) for i, k in zip(infos, keep)) and "bbox" not in infos[0]
    for f in range(3):
        a, b = start[f], start[f + 1]
        assert np.array_equal(out[f]["name"], infos[f]["name"]) and np.array_equal(out[f]["score"], infos[f]["score"])
        for k in KEYS:
            assert out[f][k].dtype == np.float32
            close(out[f][k], g["cam_out_" + k][a:b], float(g["tol_" + k]), "camera_keys %s of frame %d" % (k, f))
        # merge's z += h / 2 before and the conversion's in-place z -= h / 2 after: float32 both
        z = g["cam_boxes"][a:b, 2] + g["cam_boxes"][a:b, 5] / 2
        assert np.array_equal(out[f]["boxes_lidar"][:, 2], z - g["cam_boxes"][a:b, 5] / np.float32(2))
    assert out[3]["bbox"].shape == (0, 4) and out[3]["boxes_lidar"].shape == (0, 7) and out[3]["alpha"].shape == (0,)
    assert K.camera_keys([], [], [], _export=R.export_host) == []


def test_waymo_prediction_dicts():
    boxes = torch.tensor([[1.0, 2.0, 0.5, 4.0, 2.0, 1.5, 0.1], [3.0, 1.0, 0.25, 0.8, 0.8, 1.7, 0.2], [5.0, 5.0, 1.0, 4.2, 1.9, 1.6, 0.3]])
    pred = [{"pred_boxes": boxes, "pred_scores": torch.tensor([0.9, 0.8, 0.7]), "pred_labels": torch.tensor([1, 2, 1])},
            {"pred_boxes": torch.zeros((0, 7)), "pred_scores": torch.zeros(0), "pred_labels": torch.zeros(0, dtype=torch.int64)}]
    batch = {"frame_id": ["a", "b"], "seq_id": ["s0", "s1"]}
    before = boxes.clone()
    annos = K.waymo_prediction_dicts(batch, pred, R.CLASSES, label_offset=0.3)
    assert torch.equal(boxes, before)
    assert list(annos[0].keys()) == ["name", "score", "boxes_lidar", "frame_id", "seq_id"]
    assert list(annos[0]["name"]) == ["Vehicle", "Pedestrian", "Vehicle"] and annos[0]["score"].dtype == np.float32
    want = before.numpy().copy()
    want[[0, 2], 2] = want[[0, 2], 2] + np.float32(0.3)
    assert annos[0]["boxes_lidar"].dtype == np.float32 and np.array_equal(annos[0]["boxes_lidar"], want)
    assert annos[1]["boxes_lidar"].shape == (0, 7) and annos[1]["boxes_lidar"].dtype == np.float64 and annos[1]["name"].shape == (0,)
    assert (annos[1]["frame_id"], annos[1]["seq_id"]) == ("b", "s1")
    assert np.array_equal(K.waymo_prediction_dicts(batch, pred, R.CLASSES)[0]["boxes_lidar"], before.numpy())

    class Back:
        def backward(self, d):
            d = dict(d)
            d["boxes_lidar"] = d["boxes_lidar"] * 2
            return d

    aug = K.waymo_prediction_dicts(batch, pred, R.CLASSES, label_offset=0.3, test_augmentor=Back())
    assert np.array_equal(aug[0]["boxes_lidar"], want * 2) and aug[0]["frame_id"] == "a"


class FakeEngine:
    """returns the golden's export inputs of frames main / second / exact for whatever it is fed, and remembers what that was"""

    def __init__(self, g):
        self.pred, self.seen = [pred_dicts_of(g)[i] for i in (0, 1, 4)], []

    def forward(self, points):
        at = len(self.seen)
        self.seen += [p.clone() for p in points]
        return self.pred[at:at + len(points)]


def kitti_directory(g, root):
    start = offsets(g["fov_n"])
    (root / "velodyne").mkdir(), (root / "calib").mkdir()
    infos = []
    for f in range(3):
        name = "%06d" % (f + 10)
        g["fov_points"][start[f]:start[f + 1]].tofile(root / "velodyne" / (name + ".bin"))
        (root / "calib" / (name + ".txt")).write_text(str(g["calib%d_text" % f]))
        infos.append({"point_cloud": {"num_features": 4, "lidar_idx": name}, "image": {"image_idx": name, "image_shape": np.array(R.IMAGE_SHAPES[f], np.int32)}})
    return infos


def test_evaluate_split_on_a_synthetic_directory(g, tmp_path):
    infos = kitti_directory(g, tmp_path)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    eng = FakeEngine(g)
    result, ret, annos = K.evaluate_split(eng, infos, tmp_path, R.CLASSES, batch=2, output_path=out_dir, _fov=R.fov_host, _export=R.export_host)
    assert result is None and ret == {} and len(annos) == 3                     # no annos in the infos: the reference's answer
    start = offsets(g["fov_n"])
    for f in range(3):
        a, b = start[f], start[f + 1]
        want = g["fov_points"][a:b][g["fov_flag"][a:b]]
        assert tuple(eng.seen[f].shape) == (len(want), 4) and np.array_equal(eng.seen[f].numpy()[:, :2], want[:, :2])
        assert annos[f]["frame_id"] == "%06d" % (f + 10) and (out_dir / ("%06d.txt" % (f + 10))).exists()
    direct = K.generate_prediction_dicts({"frame_id": ["x"] * 3, "calib": [calib_of(g, i) for i in range(3)], "image_shape": R.IMAGE_SHAPES},
                                         eng.pred, R.CLASSES, _export=R.export_host)
    for a, d in zip(annos, direct):
        assert all(np.array_equal(a[k], d[k]) for k in ANNO_KEYS[:-1])
    for info, a in zip(infos, annos):
        info["annos"] = {"name": a["name"], "marker": len(a["score"])}
    seen = {}

    def evaluate(det, gt, classes):
        seen.update(det=det, gt=gt, classes=classes)
        return "AP", {"x": 1.0}

    result, ret, annos2 = K.evaluate_split(FakeEngine(g), infos, str(tmp_path), R.CLASSES, batch=3, _fov=R.fov_host, _export=R.export_host, _evaluate=evaluate)
    assert (result, ret) == ("AP", {"x": 1.0}) and seen["classes"] == R.CLASSES
    assert [x["marker"] for x in seen["gt"]] == [len(a["score"]) for a in annos2] and len(seen["det"]) == 3
    assert all(np.array_equal(x["bbox"], y["bbox"]) for x, y in zip(annos, annos2))


def test_public_signatures_are_the_references():
    def names(fn):
        return [p for p in inspect.signature(fn).parameters if not p.startswith("_")]

    assert names(K.generate_prediction_dicts) == ["batch_dict", "pred_dicts", "class_names", "output_path"]
    assert inspect.signature(K.generate_prediction_dicts).parameters["output_path"].default is None
    assert names(K.fov_points) == ["points_list", "calibs", "image_shapes", "z_shift", "num_features"]
    assert names(K.camera_keys) == ["infos", "calibs", "image_shapes"]
    assert names(K.evaluation) == ["det_annos", "gt_annos", "class_names"]
    assert names(K.evaluate_split) == ["engine", "infos", "root_path", "class_names", "batch", "output_path"]
    assert names(K.waymo_prediction_dicts) == ["batch_dict", "pred_dicts", "class_names", "label_offset", "test_augmentor"]
    assert names(K.Calibration.__init__) == ["self", "calib_file"]
    assert names(K.boxes3d_lidar_to_kitti_camera) == ["boxes3d_lidar", "calib"] and names(K.boxes3d_kitti_camera_to_lidar) == ["boxes3d_camera", "calib"]
    assert names(K.boxes3d_kitti_camera_to_imageboxes) == ["boxes3d", "calib", "image_shape"] and names(K.get_fov_flag) == ["pts_rect", "img_shape", "calib"]
