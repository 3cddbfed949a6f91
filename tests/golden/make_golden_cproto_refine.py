#!/usr/bin/env python3
"""Golden vectors of the C_PROTO refiner's second half, computed by the REFERENCE itself (build container only).

cpd/unsupervised_core/c_proto_refine.py and outline_utils.py are imported from the reference tree by path, as
make_golden_cproto.py does. The input is cpd_amd.synthetic.cproto_sequence(SEED, dtypes=DTYPES): five sweeps mixing float16 and
float32 (regenerated from the seed by the tests; a digest is stored), written to a temporary directory as the dataset stores a
sequence and run through the reference's whole C_PROTO.__call__ (ground_removal's argsort made stable, §5l). The config is the
first golden's (BasicProtoScoreThresh lowered, the Cyclist's raised above every score so that the class keeps no prototype and
its boxes take the predefined size) with OrienThresh = 0.62, inside the range of the synthetic vehicles' scores, and the yaml's
StaticThresh.

Stored (data only): the seed and the digest; the reference's own _CSS.pkl contents and the basic / high-quality prototypes of its
_CSS_proto.pkl -- the tests' INPUT, so the first stage's cell-count differences do not leak in; the _resize infos (box, score,
proto id); the final infos (box, cls, score, proto id); per segment (a box of a class the refiner takes, frame-major) where it
is, its fit_index kind, whether a cluster was found and whether the restatement's cell counts are the reference's; per Vehicle
segment with a cluster the branch and side correct_orientation took (restatement), the reference's score and a flag where the
restatement's box differs from the reference's by more than 1e-9.
Asserted: see the end of main().
Usage:  python tests/golden/make_golden_cproto_refine.py
"""
import copy
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import make_golden_cproto as MG  # noqa: E402

REF = MG.REF
SEED, N_AZ = 31, 1100
DTYPES = (np.float16, np.float32, np.float16, np.float32, np.float16)
SEQ = "segment-12345678_refine"
THRESH = {'Vehicle': 0.55, 'Pedestrian': 0.6, 'Cyclist': 2.0}
ORIEN_THRESH, STATIC_THRESH = 0.62, 0.8


def golden_config():
    cfg = MG.golden_config()
    cfg["RefinerConfig"]["BasicProtoScoreThresh"] = dict(THRESH)
    cfg["RefinerConfig"]["OrienThresh"] = ORIEN_THRESH
    cfg["RefinerConfig"]["StaticThresh"] = STATIC_THRESH
    return cfg


def sequence(seed=SEED, n_az=N_AZ):
    from cpd_amd import synthetic
    return synthetic.cproto_sequence(seed, n_az=n_az, dtypes=DTYPES)


def pack_tables(ps):
    """The part of a _CSS_proto.pkl that refine_box_size reads, in insertion order."""
    from cpd_amd.cproto import CLASSES
    keys, whl = [], []
    for ci, c in enumerate(CLASSES):
        for pid, v in ps['basic_proto_set'][c].items():
            keys.append((ci, pid)), whl.append(v)
    out = dict(basic_key=np.array(keys, np.int64).reshape(-1, 2), basic_whl=np.array(whl, np.float64).reshape(-1, 3))
    keys, box = [], []
    for ci, c in enumerate(CLASSES):
        for pid, v in ps['high_quality_proto_set'][c].items():
            keys.append((ci, pid)), box.append(v['box'])
    out["hq_key"], out["hq_box"] = np.array(keys, np.int64).reshape(-1, 2), np.array(box, np.float64).reshape(-1, 7)
    return out


def unpack_tables(z):
    from cpd_amd.cproto import CLASSES
    ps = {'basic_proto_set': {c: {} for c in CLASSES}, 'high_quality_proto_set': {c: {} for c in CLASSES},
          'proto_points_set': {c: {} for c in CLASSES}}
    for (ci, pid), whl in zip(z["basic_key"], z["basic_whl"]):
        ps['basic_proto_set'][CLASSES[int(ci)]][int(pid)] = whl.copy()
    for (ci, pid), box in zip(z["hq_key"], z["hq_box"]):
        ps['high_quality_proto_set'][CLASSES[int(ci)]][int(pid)] = {'box': box.copy()}
    return ps


def unpack_infos(z, prefix, seq_infos, with_cls=False):
    """The info list of one stored stage on top of the regenerated sequence's ids and poses."""
    infos = []
    for i, src in enumerate(seq_infos):
        d = dict(outline_box=z["%s%d_box" % (prefix, i)].copy(), outline_score=z["%s%d_score" % (prefix, i)].copy(),
                 outline_ids=src['outline_ids'].copy(), outline_cls=src['outline_cls'].copy(), pose=src['pose'].copy())
        if "%s%d_pid" % (prefix, i) in z:
            d['outline_proto_id'] = z["%s%d_pid" % (prefix, i)].copy()
        if with_cls:
            d['outline_cls'] = z["%s%d_cls" % (prefix, i)].astype(src['outline_cls'].dtype)
        infos.append(d)
    return infos


def main():
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    from cpd_amd.cproto import CLASSES
    import ref_cproto as R
    import ref_cproto_refine as RR
    sys.path.insert(0, REF)
    import cpd.unsupervised_core.ground_removal as gr
    import cpd.unsupervised_core.outline_utils as ou
    import cpd.unsupervised_core.c_proto_refine as cp

    cfg = golden_config()
    ns = MG.namespace(cfg)
    frames, infos = sequence()
    out = dict(seed=np.array(SEED), n_az=np.array(N_AZ), seq=np.array(SEQ), digest=np.array(MG.digest(frames, infos)),
               thresh=np.array([THRESH[c] for c in CLASSES]), orien_thresh=np.array(ORIEN_THRESH),
               static_thresh=np.array(STATIC_THRESH))

    # 1. the reference's whole refiner (stable argsort)
    unstable_np = gr.np
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, SEQ))
        for i, f in enumerate(frames):
            np.save(os.path.join(root, SEQ, "%04d.npy" % i), f)
        with open(os.path.join(root, SEQ, SEQ + "_outline_MFCF.pkl"), "wb") as f:
            pickle.dump(infos, f)
        gr.np = MG._StableNumpy()
        try:
            final = cp.C_PROTO(SEQ, root, ns)()
        finally:
            gr.np = unstable_np
        load = lambda name: pickle.load(open(os.path.join(root, SEQ, SEQ + "_outline_" + name + ".pkl"), "rb"))
        css, proto, resize = load("MFCF_CSS"), load("MFCF_CSS_proto"), load("C_PROTO_resize")
        for a, b in zip(final, load("C_PROTO")):
            assert np.array_equal(a['outline_box'], b['outline_box'])

    # 2. the restatement from the reference's own _CSS infos and prototypes, segment by segment
    tables = RR.hq_tables(proto)
    parts = cfg["RefinerConfig"]["CSSConfig"]["MLOParts"]
    seg = dict(where=[], fit=[], has=[], occ_same=[])
    veh = dict(where=[], branch=[], side=[], score_ref=[], flag=[], worst=[])
    seq_id = int(SEQ[8:16])
    for i, info in enumerate(css):
        xyz = frames[i][:, 0:3]
        for b in range(len(info['outline_box'])):
            name = info['outline_cls'][b]
            if name not in CLASSES:
                assert np.array_equal(resize[i]['outline_box'][b], info['outline_box'][b]) and resize[i]['outline_proto_id'][b] == -1
                continue
            s = R.segment(xyz, info['outline_box'][b], cfg)
            r = RR.refine_segment(xyz, info['outline_box'][b], name, int(str(seq_id) + str(info['outline_ids'][b])), tables, cfg, s)
            what = "frame %d box %d: " % (i, b)
            assert r["proto_id"] == resize[i]['outline_proto_id'][b], what + "proto id"
            has = r["score"] is not None
            occ_same = True
            if has:
                occ_ref = [int(round(ou.compute_confidence(s["cluster"], r["fitted"], p) * p * p)) for p in parts]
                occ_same = occ_ref == list(r["occ"])
                if occ_same:
                    assert abs(r["score"] - resize[i]['outline_score'][b]) <= 1e-12, what + "score"
            else:
                assert resize[i]['outline_score'][b] == info['outline_score'][b], what + "score of a box without a cluster"
            seg["where"].append((i, b)), seg["fit"].append(r["fit_index"]), seg["has"].append(has)
            seg["occ_same"].append(occ_same)
            dif = float(np.abs(r["box"] - resize[i]['outline_box'][b]).max())
            if name == 'Vehicle' and has:
                # the reference's own choice between the two boxes goes by its own score
                mine = r["box_orient_drift"] if resize[i]['outline_score'][b] > ORIEN_THRESH else r["box_drift"]
                dif = float(np.abs(mine - resize[i]['outline_box'][b]).max())
                if (r["score"] > ORIEN_THRESH) != (resize[i]['outline_score'][b] > ORIEN_THRESH):
                    assert not occ_same
                veh["where"].append((i, b)), veh["branch"].append(r["orient"]["branch"] == 'x')
                veh["side"].append(r["orient"]["side"] == 'max'), veh["score_ref"].append(resize[i]['outline_score'][b])
                veh["flag"].append(dif > 1e-9), veh["worst"].append(dif)
            else:
                assert dif <= 1e-9, what + "box of a segment without orientation / drift (%g)" % dif

    # 3. refine_box_pos: the restatement and the product's host code from the reference's _resize infos
    from cpd_amd import cproto_refine
    pos, static_ids, dynamic = RR.refine_box_pos(resize, cfg)
    prod = cproto_refine.refine_box_pos(copy.deepcopy(resize), cfg["RefinerConfig"])
    changed = False
    for a, p, b, r0 in zip(pos, prod, final, resize):
        for got in (a, p):
            assert np.abs(got['outline_box'] - b['outline_box']).max() <= 1e-9
            assert np.array_equal(got['outline_cls'], b['outline_cls']) and np.array_equal(got['outline_proto_id'], b['outline_proto_id'])
            assert np.abs(got['outline_score'] - b['outline_score']).max() <= 1e-12
        changed |= bool((b['outline_cls'] != r0['outline_cls']).any() or (b['outline_score'] != r0['outline_score']).any())

    n_veh, n_flag = len(veh["flag"]), int(np.sum(veh["flag"]))
    score = np.array(veh["score_ref"])
    print("%d segments, %d with a cluster, %d vehicle segments with a cluster, %d flagged (worst unflagged %.3g); fit kinds %s; "
          "branch x %d / y %d, side max %d / min %d; scores %.3f..%.3f, %d above OrienThresh; static %s dynamic %s" % (
              len(seg["fit"]), int(np.sum(seg["has"])), n_veh, n_flag,
              max([w for w, f in zip(veh["worst"], veh["flag"]) if not f], default=0.0),
              {k: int(np.sum(np.array(seg["fit"]) == k)) for k in (-2, -1)} | {"hq": int(np.sum(np.array(seg["fit"]) >= 0))},
              int(np.sum(veh["branch"])), n_veh - int(np.sum(veh["branch"])), int(np.sum(veh["side"])),
              n_veh - int(np.sum(veh["side"])), score.min(), score.max(), int((score > ORIEN_THRESH).sum()), static_ids,
              sorted(dynamic)))
    assert n_veh >= 20, "fewer than 20 Vehicle segments with a cluster"
    assert n_flag <= 0.05 * n_veh, "%d of %d vehicle segments flagged" % (n_flag, n_veh)
    assert 0 < np.sum(veh["branch"]) < n_veh and 0 < np.sum(veh["side"]) < n_veh, "both branches and both sides must occur"
    assert 0 < (score > ORIEN_THRESH).sum() < n_veh, "scores must fall on both sides of OrienThresh"
    fit = np.array(seg["fit"])
    assert (fit == -2).any() and (fit == -1).any() and (fit >= 0).any(), "all three fit_index kinds must occur"
    assert not all(seg["has"]), "a box of a taken class without a cluster must occur"
    assert any(not h and not np.array_equal(resize[i]['outline_box'][b], css[i]['outline_box'][b])
               for (i, b), h in zip(seg["where"], seg["has"])), "a box without a cluster must still change"
    assert static_ids and dynamic, "static and dynamic tracks must both occur"
    assert changed, "a static track must rewrite a class or a score"

    for i in range(len(frames)):
        out["css%d_box" % i], out["css%d_score" % i] = css[i]['outline_box'], css[i]['outline_score']
        out["resize%d_box" % i], out["resize%d_score" % i] = resize[i]['outline_box'], resize[i]['outline_score']
        out["resize%d_pid" % i] = resize[i]['outline_proto_id']
        out["final%d_box" % i], out["final%d_score" % i] = final[i]['outline_box'], final[i]['outline_score']
        out["final%d_pid" % i], out["final%d_cls" % i] = final[i]['outline_proto_id'], np.array(final[i]['outline_cls'], 'U16')
        assert np.array_equal(css[i]['outline_cls'], infos[i]['outline_cls']) and np.array_equal(css[i]['pose'], infos[i]['pose'])
    out.update(pack_tables(proto))
    out.update(seg_where=np.array(seg["where"], np.int32), seg_fit=np.array(seg["fit"], np.int32), seg_has=np.array(seg["has"]), seg_occ_same=np.array(seg["occ_same"]),
               veh_where=np.array(veh["where"], np.int32), veh_branch_x=np.array(veh["branch"]),
               veh_side_max=np.array(veh["side"]), veh_score_ref=score, veh_flag=np.array(veh["flag"]),
               static_ids=np.array(static_ids, np.int64), dynamic_ids=np.array(sorted(dynamic), np.int64))
    path = os.path.join(HERE, "cproto_refine.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
