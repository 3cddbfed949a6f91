#!/usr/bin/env python3
"""Golden vectors of the C_PROTO refiner's first stage, computed by the REFERENCE itself (build container only).

cpd/unsupervised_core/c_proto_refine.py and outline_utils.py are imported from the reference tree by path (numpy 2 removed
np.mat: it is aliased to np.asmatrix first). The input is cpd_amd.synthetic.cproto_sequence(SEED) (regenerated from the seed
by the tests; a digest is stored), written to a temporary directory as the dataset stores a sequence (NNNN.npy frames,
<seq>_outline_MFCF.pkl) and run through the reference's C_PROTO.compute_css_score_and_raw_proto and construct_prototypes. The
config is the cproto yaml's with BasicProtoScoreThresh lowered to 0.55 / 0.6 / 0.6, so that the synthetic boxes (scores 0.42 ..
0.87) fall on both sides of it.

Every box is also walked through the reference's own functions one stage at a time (crop expression, smooth_points,
OutlineFitter.remove_ground with ground_removal's np.argsort made stable, clustering, compute_confidence, CSS) to record the
intermediates; that walk must reproduce the driver's scores, boxes and raw prototypes exactly.
Asserted:
  (a) the restatement (tests/ref_cproto.py) equals the reference on every mask, integer, z_min and new_box (bit for bit), and
      on the score to 1e-12 -- except the cell counts and scores of the boxes it flags;
  (b) the flagged boxes (LAPACK's float32 inverse or BLAS's accumulation moves a point across a cell bound) are at most 5 %
      of the scored boxes, of which there are at least 20;
  (c) an unpatched run (unstable argsort) gives the same non-ground sets.
Stored per segment (= box of a class the refiner takes, frame-major): where it is, the crop rows, masks, z_min, new_box, the
non-ground rows in canonical order, labels, the chosen cluster, occ of the reference and of the restatement, both scores, the
flag; then the CSS infos, the raw prototypes entry by entry and construct_prototypes' output.
Usage:  python tests/golden/make_golden_cproto.py
"""
import copy
import hashlib
import os
import pickle
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("CPD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

SEED, N_AZ = 31, 1100
SEQ = "segment-12345678_golden"
THRESH = {'Vehicle': 0.55, 'Pedestrian': 0.6, 'Cyclist': 0.6}


def golden_config():
    from cpd_amd.cproto import CPROTO_CONFIG
    cfg = copy.deepcopy(CPROTO_CONFIG)
    cfg["RefinerConfig"]["BasicProtoScoreThresh"] = dict(THRESH)
    return cfg


def namespace(cfg):
    """The attribute-style config the reference reads (dict-valued leaves stay dicts)."""
    r = cfg["RefinerConfig"]
    return types.SimpleNamespace(
        InitLabelGenerator=cfg["InitLabelGenerator"], LabelRefiner=cfg["LabelRefiner"],
        GeneratorConfig=types.SimpleNamespace(**cfg["GeneratorConfig"]),
        RefinerConfig=types.SimpleNamespace(**dict(r, CSSConfig=types.SimpleNamespace(**r["CSSConfig"]))))


def digest(frames, infos):
    h = hashlib.sha256()
    for f, i in zip(frames, infos):
        h.update(np.ascontiguousarray(f).tobytes())
        h.update(np.ascontiguousarray(i['outline_box']).tobytes())
        h.update(np.ascontiguousarray(i['outline_ids']).tobytes())
        h.update(np.ascontiguousarray(i['pose']).tobytes())
        h.update("|".join(i['outline_cls']).encode())
    return h.hexdigest()


def pack_raw(raw, prov):
    """Raw prototypes entry by entry in insertion order: class index, id, (frame, box) of every entry, points as float32."""
    from cpd_amd.cproto import CLASSES
    key, n_ent, where, n_pts, pts, box, pose, score, gp = [], [], [], [], [], [], [], [], []
    for ci, c in enumerate(CLASSES):
        for pid, e in raw[c].items():
            key.append((ci, pid))
            n_ent.append(len(e['score']))
            for k in range(len(e['score'])):
                p = np.asarray(e['points'][k])
                assert np.array_equal(p.astype(np.float32).astype(np.float64), p.astype(np.float64))
                where.append(prov[(c, pid)][k])
                n_pts.append(len(p)), pts.append(p.astype(np.float32)), box.append(e['outline_box'][k])
                pose.append(e['pose'][k]), score.append(e['score'][k]), gp.append(np.asarray(e['global_position'][k]))
    return dict(raw_key=np.array(key, np.int64).reshape(-1, 2), raw_n_ent=np.array(n_ent, np.int32),
                raw_where=np.array(where, np.int32).reshape(-1, 2), raw_n_pts=np.array(n_pts, np.int32),
                raw_pts=np.concatenate(pts, 0), raw_box=np.array(box), raw_pose=np.array(pose), raw_score=np.array(score),
                raw_gp=np.array(gp, np.float32).reshape(-1, 3))


def unpack_raw(z):
    """The raw_proto_set dict back from pack_raw's arrays (first entries float64 as the reference stores them)."""
    from cpd_amd.cproto import CLASSES
    raw = {c: {} for c in CLASSES}
    e, o = 0, 0
    for (ci, pid), n in zip(z["raw_key"], z["raw_n_ent"]):
        d = raw[CLASSES[int(ci)]][int(pid)] = {'points': [], 'outline_box': [], 'pose': [], 'score': [], 'global_position': []}
        for k in range(int(n)):
            p = z["raw_pts"][o:o + z["raw_n_pts"][e]]
            d['points'].append(p.astype(np.float64) if k == 0 else p.copy())
            d['outline_box'].append(z["raw_box"][e].copy()), d['pose'].append(z["raw_pose"][e].copy())
            d['score'].append(float(z["raw_score"][e])), d['global_position'].append(z["raw_gp"][e].reshape(1, 3).copy())
            o += z["raw_n_pts"][e]
            e += 1
    return raw


def pack_proto(ps):
    from cpd_amd.cproto import CLASSES
    out = {}
    keys, whl = [], []
    for ci, c in enumerate(CLASSES):
        for pid, v in ps['basic_proto_set'][c].items():
            keys.append((ci, pid)), whl.append(v)
    out["basic_key"], out["basic_whl"] = np.array(keys, np.int64).reshape(-1, 2), np.array(whl).reshape(-1, 3)
    keys, box = [], []
    for ci, c in enumerate(CLASSES):
        for pid, v in ps['high_quality_proto_set'][c].items():
            keys.append((ci, pid)), box.append(v['box'])
    out["hq_key"], out["hq_box"] = np.array(keys, np.int64).reshape(-1, 2), np.array(box).reshape(-1, 7)
    keys, box, score, move, n, pts = [], [], [], [], [], []
    for ci, c in enumerate(CLASSES):
        for pid, v in ps['proto_points_set'][c].items():
            p = np.asarray(v['points'])
            assert np.array_equal(p.astype(np.float32).astype(np.float64), p.astype(np.float64))
            keys.append((ci, pid)), box.append(v['box']), score.append(v['score']), move.append(v['move'])
            n.append(len(p)), pts.append(p.astype(np.float32))
    out["pp_key"], out["pp_box"] = np.array(keys, np.int64).reshape(-1, 2), np.array(box).reshape(-1, 7)
    out["pp_score"], out["pp_move"], out["pp_n"] = np.array(score), np.array(move, np.int8), np.array(n, np.int32)
    out["pp_pts"] = np.concatenate(pts, 0) if pts else np.zeros((0, 3), np.float32)
    return out


class _StableNumpy(types.ModuleType):
    def __init__(self):
        super().__init__("numpy_stable_argsort")

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kw):
        return np.argsort(a, kind="stable")


def main():
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    from cpd_amd import synthetic
    from cpd_amd.cproto import CLASSES
    import ref_cproto as R
    sys.path.insert(0, REF)
    import cpd.unsupervised_core.ground_removal as gr
    import cpd.unsupervised_core.outline_utils as ou
    import cpd.unsupervised_core.c_proto_refine as cp

    cfg = golden_config()
    ns = namespace(cfg)
    frames, infos = synthetic.cproto_sequence(SEED, n_az=N_AZ)
    out = dict(seed=np.array(SEED), n_az=np.array(N_AZ), seq=np.array(SEQ), digest=np.array(digest(frames, infos)),
               thresh=np.array([THRESH[c] for c in CLASSES]), n_points=np.array([len(f) for f in frames], np.int32))
    unstable_np, stable_np = gr.np, _StableNumpy()

    # 1. the reference's driver, end to end (stable argsort), then construct_prototypes
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, SEQ))
        for i, f in enumerate(frames):
            np.save(os.path.join(root, SEQ, "%04d.npy" % i), f)
        with open(os.path.join(root, SEQ, SEQ + "_outline_MFCF.pkl"), "wb") as f:
            pickle.dump(infos, f)
        gr.np = stable_np
        try:
            driver = cp.C_PROTO(SEQ, root, ns)
            ref_infos = driver.compute_css_score_and_raw_proto()
        finally:
            gr.np = unstable_np
        with open(os.path.join(root, SEQ, SEQ + "_outline_MFCF_CSS_raw_proto.pkl"), "rb") as f:
            ref_raw = pickle.load(f)
        ref_proto = driver.construct_prototypes()

    # 2. box by box through the reference's functions, recording every stage; the restatement beside it
    fitter, css = driver.outline_estimator, driver.css_estimator
    parts = cfg["RefinerConfig"]["CSSConfig"]["MLOParts"]
    predefined = cfg["RefinerConfig"]["CSSConfig"]["PredifinedSize"]
    seq_id = int(SEQ[8:16])
    walk_infos = copy.deepcopy(infos)
    raw, prov = {c: {} for c in CLASSES}, {}
    seg = dict(where=[], n_crop=[], crop_src=[], dens=[], z_min=[], new_box=[], had=[], n_filt=[], filt_src=[], n_ng=[],
               ng_src=[], labels=[], best_label=[], best_count=[], cluster_src=[], occ_ref=[], occ=[], score_ref=[], score=[],
               flag=[])
    n_scored = 0
    for i, info in enumerate(walk_infos):
        xyz = frames[i][:, 0:3]
        score_i = np.zeros(shape=info['outline_cls'].shape)
        for b in range(len(info['outline_box'])):
            name = info['outline_cls'][b]
            if name not in raw:
                continue
            box = R.presize(info['outline_box'][b], name, predefined)
            info['outline_box'][b] = box
            r = R.segment(xyz, box, cfg)
            # the reference, stage by stage
            dis = np.sqrt(np.sum((xyz[:, 0:2] - box[0:2]) ** 2, -1))
            crop_src = np.nonzero(dis < (max(box[3], box[4])))[0]
            low = xyz[crop_src]
            dens = np.zeros(0, bool)
            if len(low) > 0:
                from scipy.spatial import cKDTree
                dens = cKDTree(low[:, 0:3]).query_ball_point(low[:, 0:3], r=0.2, return_length=True) > 3
                assert np.array_equal(ou.smooth_points(low), low[dens])
            low_src, low = crop_src[dens], low[dens]
            z_min = min(low[:, 2]) if len(low) > 0 else box[2] - box[5] / 2
            z_max = box[2] + box[5] / 2
            h = z_max - z_min
            if h < 1.3:
                h = 1.3
            new_box = np.array([box[0], box[1], h / 2 + z_min, box[3], box[4], h, box[6]])
            filt_src = ng_src = labels = cluster_src = np.zeros(0, np.int64)
            best_label, best_count, occ_ref, score_ref = -1, 0, np.zeros(len(parts), np.int32), 0.0
            if len(low) > 0:
                mask = (low[:, 2] > z_min + 0.2) * (low[:, 2] < z_max)
                low, filt_src = low[mask], low_src[mask]
                gr.np = stable_np
                try:
                    ng = fitter.remove_ground(low)
                finally:
                    gr.np = unstable_np
                ng_u = fitter.remove_ground(low)
                assert np.array_equal(np.unique(ng, axis=0), np.unique(ng_u, axis=0)) and len(ng) == len(ng_u), \
                    "(c) the non-ground set depends on the sort (frame %d box %d)" % (i, b)
                assert np.array_equal(ng, xyz[r["ng_src"]].astype(np.float64)), \
                    "(a) non-ground rows / order (frame %d box %d)" % (i, b)
                ng_src = r["ng_src"]
                if len(ng) > 10:
                    clusters, _ = fitter.clustering(ng)
                    labels = fitter.cluster_method.labels_.astype(np.int64)
                    if len(clusters) > 0:
                        max_cluter = clusters[0]
                        for clu in clusters:
                            if len(clu) > len(max_cluter):
                                max_cluter = clu
                        lab_ids = [l for l in range(labels.max() + 1) if len(ng[labels == l]) == len(max_cluter)
                                   and np.array_equal(ng[labels == l], max_cluter)]
                        best_label, best_count = lab_ids[0], len(max_cluter)
                        cluster_src = ng_src[labels == best_label]
                        occ_ref = np.array([int(round(ou.compute_confidence(max_cluter, new_box, p) * p * p)) for p in parts],
                                           np.int32)
                        score_ref = css(max_cluter, new_box, name)
                        score_i[b] = score_ref
                        info['outline_box'][b] = new_box
                        n_scored += 1
                        if score_ref > THRESH[name]:
                            pid = int(str(seq_id) + str(info['outline_ids'][b]))
                            gp = ou.points_rigid_transform([new_box[0:3]], info['pose'])[0:, 0:3]
                            if pid in raw[name]:
                                e = raw[name][pid]
                                pose_i = np.linalg.inv(e['pose'][0])
                                e['points'].append(ou.points_rigid_transform(ou.points_rigid_transform(max_cluter, info['pose']),
                                                                             pose_i))
                                e['outline_box'].append(new_box), e['pose'].append(info['pose'])
                                e['score'].append(score_ref), e['global_position'].append(gp)
                            else:
                                raw[name][pid] = {'points': [max_cluter], 'outline_box': [new_box], 'pose': [info['pose']],
                                                  'score': [score_ref], 'global_position': [gp]}
                            prov.setdefault((name, pid), []).append((i, b))
            # (a) restatement against the reference
            what = "(a) frame %d box %d: " % (i, b)
            assert np.array_equal(r["crop_src"], crop_src), what + "crop"
            assert np.array_equal(r["dens_mask"], dens), what + "density mask"
            assert r["z_min"] == float(z_min) and np.array_equal(r["new_box"], new_box), what + "z_min / new_box"
            assert r["had_points"] == (len(low_src) > 0) and np.array_equal(r["filt_src"], filt_src), what + "window"
            assert np.array_equal(r["labels"], labels), what + "labels"
            assert r["best_label"] == best_label and r["best_count"] == best_count, what + "chosen cluster"
            assert np.array_equal(r["cluster_src"], cluster_src), what + "cluster rows"
            flag = not np.array_equal(r["occ"], occ_ref)
            score = R.css_from_occ(r["occ"], new_box, name, cfg["RefinerConfig"]["CSSConfig"]) if best_label >= 0 else 0.0
            if not flag:
                assert abs(score - score_ref) <= 1e-12, what + "score"
            if flag:
                assert (score > THRESH[name]) == (score_ref > THRESH[name]), what + "a flagged box crosses the threshold"
            seg["where"].append((i, b)), seg["n_crop"].append(len(crop_src)), seg["crop_src"].append(crop_src)
            seg["dens"].append(dens), seg["z_min"].append(float(z_min)), seg["new_box"].append(new_box)
            seg["had"].append(len(low_src) > 0), seg["n_filt"].append(len(filt_src)), seg["filt_src"].append(filt_src)
            seg["n_ng"].append(len(ng_src)), seg["ng_src"].append(ng_src), seg["labels"].append(labels)
            seg["best_label"].append(best_label), seg["best_count"].append(best_count), seg["cluster_src"].append(cluster_src)
            seg["occ_ref"].append(occ_ref), seg["occ"].append(r["occ"]), seg["score_ref"].append(score_ref)
            seg["score"].append(score), seg["flag"].append(flag)
        info['outline_score'] = score_i

    # 3. the walk is the driver
    for a, b in zip(walk_infos, ref_infos):
        assert np.array_equal(a['outline_box'], b['outline_box']) and np.array_equal(a['outline_score'], b['outline_score'])
    for c in CLASSES:
        assert list(raw[c]) == list(ref_raw[c])
        for pid in raw[c]:
            for k in ('points', 'outline_box', 'pose', 'score', 'global_position'):
                assert len(raw[c][pid][k]) == len(ref_raw[c][pid][k])
                assert all(np.array_equal(x, y) for x, y in zip(raw[c][pid][k], ref_raw[c][pid][k])), (c, pid, k)
    n_flag = int(np.sum(seg["flag"]))
    print("%d segments, %d scored, %d flagged; raw prototypes per class %s; moving %s" % (
        len(seg["flag"]), n_scored, n_flag, {c: {p: len(e['score']) for p, e in raw[c].items()} for c in CLASSES},
        {c: [p for p, v in ref_proto['proto_points_set'][c].items() if v['move']] for c in CLASSES}))
    assert n_scored >= 20, "(b) fewer than 20 scored boxes"
    assert n_flag <= 0.05 * n_scored, "(b) %d of %d scored boxes flagged" % (n_flag, n_scored)
    assert any(v['move'] for c in CLASSES for v in ref_proto['proto_points_set'][c].values())
    assert any(len(e['score']) > 1 and not ref_proto['proto_points_set'][c][p]['move'] for c in CLASSES for p, e in raw[c].items())

    cat = lambda v, dt: np.concatenate([np.asarray(x, dt) for x in v]) if v else np.zeros(0, dt)
    out.update(seg_where=np.array(seg["where"], np.int32), seg_n_crop=np.array(seg["n_crop"], np.int32),
               seg_crop_src=cat(seg["crop_src"], np.int32), seg_dens=np.packbits(cat(seg["dens"], bool)),
               seg_z_min=np.array(seg["z_min"]), seg_new_box=np.array(seg["new_box"]), seg_had=np.array(seg["had"]),
               seg_n_filt=np.array(seg["n_filt"], np.int32), seg_filt_src=cat(seg["filt_src"], np.int32),
               seg_n_ng=np.array(seg["n_ng"], np.int32), seg_ng_src=cat(seg["ng_src"], np.int32),
               seg_n_lab=np.array([len(l) for l in seg["labels"]], np.int32), seg_labels=cat(seg["labels"], np.int16),
               seg_best_label=np.array(seg["best_label"], np.int32), seg_best_count=np.array(seg["best_count"], np.int32),
               seg_cluster_src=cat(seg["cluster_src"], np.int32), seg_occ_ref=np.array(seg["occ_ref"], np.int32),
               seg_occ=np.array(seg["occ"], np.int32), seg_score_ref=np.array(seg["score_ref"], np.float64),
               seg_score=np.array(seg["score"], np.float64), seg_flag=np.array(seg["flag"]))
    for i, info in enumerate(ref_infos):
        out["info%d_box" % i], out["info%d_score" % i] = info['outline_box'], info['outline_score']
    out.update(pack_raw(ref_raw, prov))
    assert all(np.array_equal(x, y) for c in CLASSES for p in ref_raw[c]
               for x, y in zip(unpack_raw(out)[c][p]['points'], ref_raw[c][p]['points']))
    out.update(pack_proto(ref_proto))
    path = os.path.join(HERE, "cproto.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
