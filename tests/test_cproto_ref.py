"""CPU: the restatement of the C_PROTO refiner's first stage (tests/ref_cproto.py) against the reference's recorded output
(tests/golden/cproto.npz, written by make_golden_cproto.py), cpd_amd.cproto's host-only parts (construct_prototypes, the CSS
formulas) and the new C-ABI entry points' host-side behaviour (no kernel is launched)."""
import copy
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import ref_cproto as R
from cpd_amd.synthetic import cproto_sequence

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_golden_cproto as MG  # noqa: E402  (helpers only: the digest, the config, the raw-prototype packing)

ENTRY_POINTS = ("cpd_cproto_crop_workspace_bytes", "cpd_cproto_crop_count", "cpd_cproto_crop_fill",
                "cpd_cproto_filter_workspace_bytes", "cpd_cproto_filter", "cpd_cproto_score_workspace_bytes", "cpd_cproto_score")


@pytest.fixture(scope="module")
def cz(golden):
    return golden("cproto")


_CACHE = {}


def golden_sequence(cz):
    """(frames, infos) of the golden sequence, regenerated from its seed and checked against the stored digest."""
    if "seq" not in _CACHE:
        frames, infos = cproto_sequence(int(cz["seed"]), n_az=int(cz["n_az"]))
        assert MG.digest(frames, infos) == str(cz["digest"]), (
            "cproto_sequence(%d) no longer reproduces the golden's input (numpy RNG or synthetic.py changed): regenerate "
            "tests/golden/cproto.npz" % int(cz["seed"]))
        _CACHE["seq"] = (frames, infos)
    frames, infos = _CACHE["seq"]
    return frames, copy.deepcopy(infos)


def golden_segments(cz):
    """The recorded stages per segment, as a list of dicts in segment order."""
    if "segs" not in _CACHE:
        def split(flat, counts):
            o = np.concatenate([[0], np.cumsum(counts)])
            return [flat[o[k]:o[k + 1]] for k in range(len(counts))]
        n_crop = cz["seg_n_crop"]
        dens = np.unpackbits(cz["seg_dens"])[:int(n_crop.sum())].astype(bool)
        cols = dict(crop_src=split(cz["seg_crop_src"], n_crop), dens_mask=split(dens, n_crop),
                    filt_src=split(cz["seg_filt_src"], cz["seg_n_filt"]), ng_src=split(cz["seg_ng_src"], cz["seg_n_ng"]),
                    labels=split(cz["seg_labels"].astype(np.int64), cz["seg_n_lab"]),
                    cluster_src=split(cz["seg_cluster_src"], cz["seg_best_count"]))
        segs = []
        for s in range(len(n_crop)):
            d = {k: v[s] for k, v in cols.items()}
            d.update(where=tuple(cz["seg_where"][s]), z_min=cz["seg_z_min"][s], new_box=cz["seg_new_box"][s],
                     had_points=bool(cz["seg_had"][s]), best_label=int(cz["seg_best_label"][s]),
                     best_count=int(cz["seg_best_count"][s]), occ_ref=cz["seg_occ_ref"][s], occ=cz["seg_occ"][s],
                     score_ref=cz["seg_score_ref"][s], score=cz["seg_score"][s], flag=bool(cz["seg_flag"][s]))
            segs.append(d)
        _CACHE["segs"] = segs
    return _CACHE["segs"]


def check_stages(got, want, what):
    """Every integer, mask, z_min and new_box (bit for bit) of one segment."""
    for k in ("crop_src", "dens_mask", "filt_src", "ng_src", "labels", "cluster_src"):
        np.testing.assert_array_equal(np.asarray(got[k]), want[k], err_msg="%s: %s" % (what, k))
    assert float(got["z_min"]) == want["z_min"], what
    assert np.array_equal(np.asarray(got["new_box"]).view(np.uint64), want["new_box"].view(np.uint64)), what
    assert bool(got["had_points"]) == want["had_points"] and int(got["best_label"]) == want["best_label"], what
    assert int(got["best_count"]) == want["best_count"], what
    np.testing.assert_array_equal(np.asarray(got["occ"]), want["occ"], err_msg="%s: occ" % what)


def test_golden_discriminates(cz):
    segs = golden_segments(cz)
    scored = [s for s in segs if s["best_label"] >= 0]
    assert len(scored) >= 20 and sum(s["flag"] for s in segs) <= 0.05 * len(scored)
    assert any(not s["had_points"] for s in segs) and any(len(s["crop_src"]) == 0 for s in segs)
    assert any(s["had_points"] and s["best_label"] < 0 for s in segs)            # dense rows but no valid cluster
    assert any(len(s["ng_src"]) < len(s["filt_src"]) for s in segs)             # the ground step removes rows
    assert any(s["labels"].max(initial=-1) >= 1 for s in segs)                   # more than one cluster in a crop
    assert {str(d) for d in (f.dtype for f in golden_sequence(cz)[0])} == {"float16", "float32"}
    thr = dict(zip(R.CLASSES, cz["thresh"]))
    _, infos = golden_sequence(cz)
    above = [s["score_ref"] > thr[infos[s["where"][0]]["outline_cls"][s["where"][1]]] for s in scored]
    assert 0 < sum(above) < len(above)
    assert cz["pp_move"].any() and (~cz["pp_move"].astype(bool)).any() and cz["raw_n_ent"].max() >= 3


@pytest.mark.parametrize("frame", [0, 1])
def test_restatement_matches_golden(cz, frame):
    frames, infos = golden_sequence(cz)
    cfg = MG.golden_config()
    predefined = cfg["RefinerConfig"]["CSSConfig"]["PredifinedSize"]
    for want in golden_segments(cz):
        i, b = want["where"]
        if i != frame:
            continue
        name = infos[i]["outline_cls"][b]
        got = R.segment(frames[i][:, 0:3], R.presize(infos[i]["outline_box"][b], name, predefined), cfg)
        check_stages(got, want, "frame %d box %d" % (i, b))
        if want["best_label"] >= 0:
            score = R.css_from_occ(got["occ"], got["new_box"], name, cfg["RefinerConfig"]["CSSConfig"])
            assert score == want["score"]
            if not want["flag"]:
                assert abs(score - want["score_ref"]) <= 1e-12


def test_brute_force_density_is_the_kd_tree_count():
    rng = np.random.default_rng(4)
    p = (rng.integers(0, 24, (400, 3)) / 32).astype(np.float16)      # a 1/32 m lattice: many pairs at the same distance
    np.testing.assert_array_equal(R.smooth_mask_brute(p), R.smooth_mask(p))


def _proto_sets_equal(got, cz):
    want = MG.pack_proto(got)
    for k in ("basic_key", "hq_key", "pp_key", "pp_move", "pp_n"):
        np.testing.assert_array_equal(want[k], cz[k], err_msg=k)
    for k in ("basic_whl", "hq_box", "pp_box", "pp_score", "pp_pts"):
        np.testing.assert_allclose(want[k], cz[k], rtol=0, atol=1e-9, err_msg=k)


def test_construct_prototypes_matches_golden(cz, tmp_path):
    from cpd_amd import cproto
    cfg = MG.golden_config()
    raw = MG.unpack_raw(cz)
    _proto_sets_equal(cproto.construct_prototypes(copy.deepcopy(raw), cfg["RefinerConfig"]), cz)
    # the method: same file contract, cached
    seq = str(cz["seq"])
    os.makedirs(tmp_path / seq)
    with open(tmp_path / seq / (seq + "_outline_MFCF_CSS_raw_proto.pkl"), "wb") as f:
        import pickle
        pickle.dump(raw, f)
    c = cproto.C_PROTO(seq, str(tmp_path), cfg)
    got = c.construct_prototypes()
    _proto_sets_equal(got, cz)
    assert os.path.exists(tmp_path / seq / (seq + "_outline_MFCF_CSS_proto.pkl"))
    os.remove(tmp_path / seq / (seq + "_outline_MFCF_CSS_raw_proto.pkl"))
    again = c.construct_prototypes()        # from the cache: the raw file is gone
    assert list(again["proto_points_set"]["Vehicle"]) == list(got["proto_points_set"]["Vehicle"])
    # the consumer: prefilter.sample_prototype reads box / points / score / move per prototype
    v = next(iter(got["proto_points_set"]["Vehicle"].values()))
    assert set(v) == {"box", "points", "score", "move"} and v["points"].shape[1] == 3 and v["box"].shape == (7,)


def test_unprovided_stages_say_what_is_missing():
    from cpd_amd import cproto
    c = cproto.C_PROTO("segment-12345678_x", "/nonexistent", MG.golden_config())
    for fn in (c.refine_box_size, c.refine_box_pos, c):
        with pytest.raises(NotImplementedError, match="correct_orientation and density_guided_drift"):
            fn()


def test_host_formulas_against_reference_literals():
    """Literals computed by the reference's KL_entropy_score and CSS (an empty cluster: mlo_score 0)."""
    from cpd_amd import cproto
    y = np.array([5.065, 1.86, 1.49])
    y = y / y.sum()
    x = np.array([4.6, 1.9, 1.6])
    assert abs(cproto.KL_entropy_score(x / x.sum(), y) - 0.9495053361063462) <= 1e-15
    x = np.array([0.7, 2.9, 1.6])
    assert cproto.KL_entropy_score(x / x.sum(), y) == 0.0 == R.KL_entropy_score(x / x.sum(), y)       # clamped at max_dif
    css = cproto.CSS(MG.golden_config()["RefinerConfig"]["CSSConfig"])
    near, far = np.array([30.5, -12.25, 0.8, 4.6, 1.9, 1.6, 0.3]), np.array([90., 10., 1., 4.6, 1.9, 1.6, 0.3])
    assert abs(css.from_occ([0, 0, 0], near, "Vehicle") - 0.5128441033584799) <= 1e-15
    assert abs(css.from_occ([0, 0, 0], far, "Vehicle") - 0.3165017787021154) <= 1e-15
    assert css.dis_score(far) == 0.0 and abs(css.dis_score(near) - (3 * 0.5128441033584799 - 0.9495053361063462)) <= 1e-15
    assert abs(css.mlo_score([81, 49, 25]) - 1.0) <= 1e-15 and abs(css.mlo_score([9, 7, 5]) - (1 / 9 + 1 / 7 + 1 / 5) / 3) <= 1e-15
    np.testing.assert_array_equal(cproto.inverse_box_rows(near[None])[0], R.inv_rows32(near))
    m = cproto.inverse_box_rows(np.array([[16.0, 8.0, 0, 4.5, 4.5, 2, 0.0]]))[0]
    np.testing.assert_array_equal(m, np.array([1, 0, 0, -16, -0.0, 1, 0, -8], np.float32))


def test_sequence_generator():
    frames, infos = cproto_sequence(3, n_az=200)
    assert [f.dtype for f in frames] == [np.float16, np.float32, np.float16] and all(f.shape[1] == 5 for f in frames)
    assert np.array_equal(frames[0], frames[2]) and not np.array_equal(infos[0]["outline_box"], infos[2]["outline_box"])
    for i in infos:
        assert i["outline_box"].shape == (len(i["outline_cls"]), 7) and i["outline_box"].dtype == np.float64
        assert i["pose"].shape == (4, 4) and len(i["outline_ids"]) == len(i["outline_cls"])
        assert set(i["outline_cls"]) == {"Vehicle", "Pedestrian", "Cyclist", "Dis_Small"}
    assert np.array_equal(infos[0]["outline_ids"], infos[2]["outline_ids"])         # ids recur on the same sweep
    shared = set(infos[0]["outline_ids"]) & set(infos[1]["outline_ids"])
    assert shared and len(shared) < len(infos[0]["outline_ids"])                     # the moving tracks, and only they
    assert not np.array_equal(infos[0]["pose"], infos[1]["pose"])


def test_abi_entry_points_and_error_codes():
    from cpd_amd import _lib
    lib = _lib.lib()
    for name in ENTRY_POINTS:                                            # (argument types: test_abi checks every row of the table)
        assert hasattr(lib, name), name
        want = ctypes.c_size_t if name.endswith("_workspace_bytes") else ctypes.c_int
        assert _lib.SIGNATURES[name][0] is want
    txt = open(os.path.join(REPO, "include", "cpd_hip.h")).read()
    assert set(re.findall(r"\b(cpd_cproto_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))) == set(ENTRY_POINTS)
    assert lib.cpd_cproto_crop_workspace_bytes(128) >= 128 * 4 and lib.cpd_cproto_crop_workspace_bytes(0) > 0
    assert lib.cpd_cproto_filter_workspace_bytes(128, 1000) >= 2 * 128 * 4
    assert lib.cpd_cproto_score_workspace_bytes(128, 1000) >= 2 * 1000 * 4
    # argument checks come before any launch: no device is needed to see them
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    parts = (ctypes.c_int32 * 4)(9, 7, 5, 3)
    assert lib.cpd_cproto_crop_count(p, 0, 3, p, 1, p, p, 1023, p, p, 4096, None) == -1       # more than 1022 segments
    assert lib.cpd_cproto_crop_count(p, 2, 3, p, 1, p, p, 4, p, p, 4096, None) == -1          # dtype
    assert lib.cpd_cproto_crop_count(p, 0, 2, p, 1, p, p, 4, p, p, 4096, None) == -1          # row stride
    assert lib.cpd_cproto_crop_count(p, 0, 3, p, 1, p, p, 4, p, p, 8, None) == -2             # workspace
    assert lib.cpd_cproto_crop_fill(p, 0, 3, p, 1, p, p, 4, None, 10, p, p, None) == -1
    assert lib.cpd_cproto_filter(p, 0, p, p, p, 4, 10, 0.0, p, p, p, p, p, p, p, p, 4096, None) == -1     # radius
    assert lib.cpd_cproto_filter(p, 0, p, p, p, 4, 10, 0.2, p, p, p, p, p, p, p, p, 16, None) == -2
    args = [p] * 10 + [4, 10, parts]
    tail = [10, 5, 4.0] + [p] * 7
    assert lib.cpd_cproto_score(*args, 5, *tail, 1 << 20, None) == -4                          # more than 4 parts values
    parts[0] = 17
    assert lib.cpd_cproto_score(*args, 3, *tail, 1 << 20, None) == -4                          # a parts value above 16
    parts[0] = 9
    assert lib.cpd_cproto_score(*args, 3, *tail, 16, None) == -2
