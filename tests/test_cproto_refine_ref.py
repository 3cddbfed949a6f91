"""CPU: the restatement of the C_PROTO refiner's second half (tests/ref_cproto_refine.py) against the reference's recorded
output (tests/golden/cproto_refine.npz, written by make_golden_cproto_refine.py), cpd_amd.cproto_refine's host-only parts
(refine_box_pos, the helpers, the prototype table) and the new C-ABI entry points' host-side behaviour (no kernel is launched)."""
import copy
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest

import ref_cproto as R
import ref_cproto_refine as RR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_golden_cproto_refine as MGR  # noqa: E402  (helpers only: the config, the sequence, the table packing)

ENTRY_POINTS = ("cpd_refine_fit_size", "cpd_refine_orient_drift_workspace_bytes", "cpd_refine_orient_drift")
CPROTO_ENTRY_POINTS = ("cpd_cproto_crop_workspace_bytes", "cpd_cproto_crop_count", "cpd_cproto_crop_fill",
                       "cpd_cproto_filter_workspace_bytes", "cpd_cproto_filter", "cpd_cproto_score_workspace_bytes",
                       "cpd_cproto_score")
CFG = MGR.golden_config()


@pytest.fixture(scope="module")
def rz(golden):
    return golden("cproto_refine")


_CACHE = {}


def golden_sequence(rz):
    """(frames, infos) of the golden sequence, regenerated from its seed and checked against the stored digest."""
    if "seq" not in _CACHE:
        frames, infos = MGR.sequence(int(rz["seed"]), int(rz["n_az"]))
        assert MGR.MG.digest(frames, infos) == str(rz["digest"]), (
            "cproto_sequence(%d) no longer reproduces the golden's input (numpy RNG or synthetic.py changed): regenerate "
            "tests/golden/cproto_refine.npz" % int(rz["seed"]))
        _CACHE["seq"] = (frames, infos)
    return _CACHE["seq"]


def golden_inputs(rz):
    """(frames, the reference's _CSS infos, its prototype tables as a _CSS_proto dict): fresh copies."""
    frames, infos = golden_sequence(rz)
    return frames, MGR.unpack_infos(rz, "css", infos), MGR.unpack_tables(rz)


def restated(rz):
    """The restatement's refine_box_size over the golden input, once: (infos, {(frame, box): segment dict})."""
    if "restated" not in _CACHE:
        frames, css, proto = golden_inputs(rz)
        segs = {}
        infos = RR.refine_box_size(frames, css, proto, CFG, int(str(rz["seq"])[8:16]), lambda i, b, r: segs.__setitem__((i, b), r))
        _CACHE["restated"] = (infos, segs)
    return _CACHE["restated"]


def flagged(rz):
    return {tuple(w) for w, f in zip(rz["veh_where"], rz["veh_flag"]) if f}


def check_resize(got, rz, segs=None):
    """_resize infos against the golden: boxes <= 1e-9 (a flagged segment: against the restatement in segs), proto ids exact,
    scores <= 1e-12 where the cell counts agree."""
    frames, _ = golden_sequence(rz)
    occ_same = {tuple(w): bool(s) for w, s in zip(rz["seg_where"], rz["seg_occ_same"])}
    flags = flagged(rz)
    for i in range(len(frames)):
        np.testing.assert_array_equal(got[i]['outline_proto_id'], rz["resize%d_pid" % i])
        assert got[i]['outline_proto_id'].dtype == np.longlong
        for b in range(len(got[i]['outline_box'])):
            want = segs[(i, b)]["box"] if (i, b) in flags else rz["resize%d_box" % i][b]
            assert np.abs(got[i]['outline_box'][b] - want).max() <= 1e-9, "frame %d box %d" % (i, b)
            if occ_same.get((i, b), True):
                assert abs(got[i]['outline_score'][b] - rz["resize%d_score" % i][b]) <= 1e-12, "frame %d box %d" % (i, b)


def check_final(got, rz):
    for i in range(len(got)):
        assert np.abs(got[i]['outline_box'] - rz["final%d_box" % i]).max() <= 1e-9
        np.testing.assert_array_equal(got[i]['outline_cls'], rz["final%d_cls" % i])
        np.testing.assert_array_equal(got[i]['outline_proto_id'], rz["final%d_pid" % i])
        assert np.abs(got[i]['outline_score'] - rz["final%d_score" % i]).max() <= 1e-12


def test_golden_discriminates(rz):
    n = len(rz["veh_flag"])
    assert n >= 20 and rz["veh_flag"].sum() <= 0.05 * n
    assert 0 < rz["veh_branch_x"].sum() < n and 0 < rz["veh_side_max"].sum() < n
    assert 0 < (rz["veh_score_ref"] > float(rz["orien_thresh"])).sum() < n
    fit = rz["seg_fit"]
    assert (fit == -2).any() and (fit == -1).any() and (fit >= 0).any()
    frames, infos = golden_sequence(rz)
    assert {str(f.dtype) for f in frames} == {"float16", "float32"} and len(frames) == 5
    moved = [not np.array_equal(rz["resize%d_box" % i][b], rz["css%d_box" % i][b]) and
             rz["resize%d_score" % i][b] == rz["css%d_score" % i][b]
             for (i, b), has in zip(rz["seg_where"], rz["seg_has"]) if not has]
    assert any(moved)                                     # no cluster: the box changes, the score does not
    assert len(rz["static_ids"]) and len(rz["dynamic_ids"])
    assert any((rz["final%d_cls" % i] != infos[i]['outline_cls']).any() or
               (rz["final%d_score" % i] != rz["resize%d_score" % i]).any() for i in range(len(frames)))


def test_restatement_matches_golden(rz):
    infos, segs = restated(rz)
    check_resize(infos, rz, segs)
    for w, bx, side in zip(rz["veh_where"], rz["veh_branch_x"], rz["veh_side_max"]):
        o = segs[tuple(w)]["orient"]
        assert (o["branch"] == 'x') == bool(bx) and (o["side"] == 'max') == bool(side)
    for w, k, has in zip(rz["seg_where"], rz["seg_fit"], rz["seg_has"]):
        assert segs[tuple(w)]["fit_index"] == k and (segs[tuple(w)]["score"] is not None) == bool(has)
    pos, static, dynamic = RR.refine_box_pos(MGR.unpack_infos(rz, "resize", golden_sequence(rz)[1]), CFG)
    check_final(pos, rz)
    assert static == list(rz["static_ids"]) and sorted(dynamic) == list(rz["dynamic_ids"])


def test_refine_box_pos_files_and_cache(rz, tmp_path, monkeypatch):
    from cpd_amd import cproto, cproto_refine
    resize = MGR.unpack_infos(rz, "resize", golden_sequence(rz)[1])
    check_final(cproto_refine.refine_box_pos(copy.deepcopy(resize), CFG["RefinerConfig"]), rz)
    static, dynamic = cproto_refine.track_prototypes(copy.deepcopy(resize), CFG["RefinerConfig"])
    assert sorted(static['box']) == list(rz["static_ids"]) and sorted(dynamic['box']) == list(rz["dynamic_ids"])
    _, _, want_dynamic = RR.refine_box_pos(resize, CFG)
    for ob_id, tr in dynamic['box'].items():       # computed as the reference does, never written back
        for f, box in tr.items():
            assert np.abs(box - want_dynamic[ob_id][f]).max() <= 1e-9
    # the method: same file contract, cached, no GPU
    monkeypatch.setattr(cproto.CProtoGPU, "__init__", lambda *a, **k: pytest.fail("refine_box_pos must not open the GPU"))
    seq = str(rz["seq"])
    os.makedirs(tmp_path / seq)
    with open(tmp_path / seq / (seq + "_outline_C_PROTO_resize.pkl"), "wb") as f:
        pickle.dump(resize, f)
    c = cproto_refine.C_PROTO(seq, str(tmp_path), CFG)
    check_final(c.refine_box_pos(), rz)
    assert os.path.exists(tmp_path / seq / (seq + "_outline_C_PROTO.pkl"))
    os.remove(tmp_path / seq / (seq + "_outline_C_PROTO_resize.pkl"))
    check_final(c.refine_box_pos(), rz)            # from the cache: the _resize file is gone
    with open(tmp_path / seq / (seq + "_outline_C_PROTO_resize.pkl"), "wb") as f:
        pickle.dump(resize, f)
    again = c.refine_box_size()                    # cached too
    np.testing.assert_array_equal(again[0]['outline_box'], resize[0]['outline_box'])


def test_host_helpers_against_reference_literals():
    """Literals computed by the reference's angle_from_vector, get_registration_angle and box_rigid_transform."""
    from cpd_amd import cproto_refine as CR
    assert abs(CR.angle_from_vector(2.0, 1.0) - 0.4636476090008061) <= 1e-15
    assert abs(CR.angle_from_vector(-2.0, 1.0) - 2.677945044588987) <= 1e-15
    a = 0.3
    rot = lambda t: np.array([[np.cos(t), -np.sin(t), 0, 0], [np.sin(t), np.cos(t), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    assert abs(CR.get_registration_angle(rot(a)) - 0.3000000000000001) <= 1e-15
    assert abs(CR.get_registration_angle(rot(-a)) - 5.983185307179586) <= 1e-15
    assert CR.get_registration_angle(np.array([[1.0000001, 0], [0.0, 1]])) == 0.0            # the clamp
    pre, cur = rot(0.3), rot(0.1)
    pre[:3, 3], cur[:3, 3] = [1200.0, -340.0, 12.0], [1206.0, -339.5, 12.0]
    box = np.array([10.0, 5.0, 1.0, 4.5, 1.9, 1.6, 0.25])
    got = CR.box_rigid_transform(box, pre, cur)
    np.testing.assert_allclose(got, [2.78737735748291, 6.988524436950684, 1.0, 4.5, 1.9, 1.6, 0.4500000000000012], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got, RR.box_rigid_transform(box, pre, cur))
    assert box[6] == 0.25                                                                   # a copy
    for k, v in (("OrienThresh", 0.5), ("StaticThresh", 0.8)):
        assert CR.REFINE_CONFIG["RefinerConfig"][k] == v
    from cpd_amd import cproto
    assert "OrienThresh" not in cproto.CPROTO_CONFIG["RefinerConfig"]
    assert CR.REFINE_CONFIG["RefinerConfig"]["GroundMin"] == cproto.CPROTO_CONFIG["RefinerConfig"]["GroundMin"]


def test_prototype_table(rz):
    from cpd_amd import cproto_refine as CR
    proto = MGR.unpack_tables(rz)
    t = CR.PrototypeTable(proto, CFG["RefinerConfig"]["CSSConfig"]["PredifinedSize"])
    basic, hq = RR.hq_tables(proto)
    assert t.count == [len(hq[c][0]) for c in R.CLASSES] and t.count[2] == 0 and t.cap == max(t.count)
    for ci, c in enumerate(R.CLASSES):
        np.testing.assert_array_equal(t.hq_whl[ci, :t.count[ci]], np.array(hq[c][1]).reshape(-1, 3))
    pid = next(iter(basic['Vehicle']))
    np.testing.assert_array_equal(t.basic_whl('Vehicle', pid), basic['Vehicle'][pid])
    assert np.isnan(t.basic_whl('Vehicle', 7)).all() and np.isnan(t.basic_whl('Cyclist', pid)).all()
    assert t.proto_id(0, -2, 99) == 99 and t.proto_id(0, -1, 99) == -1 and t.proto_id(0, 1, 99) == hq['Vehicle'][0][1]
    np.testing.assert_array_equal(t.predefined[1], [1.0, 1.0, 2.0])
    many = {'basic_proto_set': {c: {} for c in R.CLASSES},
            'high_quality_proto_set': {c: {k: {'box': np.ones(7)} for k in range(65 if c == 'Vehicle' else 1)} for c in R.CLASSES}}
    with pytest.raises(NotImplementedError, match="64"):
        CR.PrototypeTable(many, CFG["RefinerConfig"]["CSSConfig"]["PredifinedSize"])


def _header_text():
    txt = open(os.path.join(REPO, "include", "cpd_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_abi_entry_points_and_error_codes():
    from cpd_amd import _lib
    lib = _lib.lib()
    txt = _header_text()
    assert set(re.findall(r"\b(cpd_refine_\w+)\s*\(", txt)) == set(ENTRY_POINTS)
    assert set(re.findall(r"\b(cpd_cproto_\w+)\s*\(", txt)) == set(CPROTO_ENTRY_POINTS)      # still exactly the seven
    for name in ENTRY_POINTS:                                            # (argument types: test_abi checks every row of the table)
        assert hasattr(lib, name), name
        want = ctypes.c_size_t if name.endswith("_workspace_bytes") else ctypes.c_int
        assert _lib.SIGNATURES[name][0] is want
    assert lib.cpd_refine_orient_drift_workspace_bytes(128) >= 128 * 8 * 4 and lib.cpd_refine_orient_drift_workspace_bytes(0) > 0
    # argument checks come before any launch: no device is needed to see them
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    count, pre = (ctypes.c_int32 * 3)(2, 0, 1), (ctypes.c_double * 9)(*range(1, 10))
    fit = lambda S=4, cap=2, count=count, pre=pre, box=p: lib.cpd_refine_fit_size(box, p, p, S, p, count, cap, pre, p, None)
    assert fit(S=1023) == -1                                         # more than 1022 segments
    assert fit(S=-1) == -1
    assert fit(cap=65) == -4 and fit(cap=0) == -4                    # more than 64 prototypes per class
    assert fit(cap=1) == -1                                          # a count above cap
    assert fit(count=(ctypes.c_int32 * 3)(0, -1, 0)) == -1
    assert fit(count=None) == -1 and fit(pre=None) == -1 and fit(box=None) == -1
    assert fit(S=0) == 0                                             # nothing to do, nothing launched
    od = lambda S=4, n=10, xyz=p, out=p, ws=p, nb=4096: lib.cpd_refine_orient_drift(xyz, p, p, p, p, S, n, out, p, p, ws, nb, None)
    assert od(S=1023) == -1 and od(n=-1) == -1 and od(xyz=None) == -1 and od(out=None) == -1
    assert od(nb=16) == -2 and od(ws=None) == -2                      # workspace
    assert od(S=0, n=0, xyz=None) == 0
