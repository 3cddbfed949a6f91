"""CPU: the restatement of generate_recall_record (tests/ref_recall.py) against the reference's own method
(tests/golden/recall.npz, made by tests/golden/make_golden_recall.py), and the host side of cpd_amd.recall.RecallRecord
(keys, summary, the distributed sum, pad_gt) with no kernel involved."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import ref_recall as R

CASES = ("plain", "one", "twice", "zero", "empty")
START = {"twice": "plain"}                       # a case that goes on from another case's dict


@pytest.fixture(scope="module")
def rz(golden):
    return golden("recall")


def case_inputs(rz, name):
    preds = R.split(rz[name + "_pred"], rz[name + "_pred_n"])
    rois = rz[name + "_rois"] if name + "_rois" in rz.files else None
    return preds, rois, rz[name + "_gt"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_method(rz, oracle, name):
    thresh = [float(t) for t in rz["thresh"]]
    assert list(rz["keys"]) == R.record_keys(thresh) == ["gt", "roi_0.3", "roi_0.5", "roi_0.7", "rcnn_0.3", "rcnn_0.5", "rcnn_0.7"]
    preds, rois, gts = case_inputs(rz, name)
    run = rz[START[name] + "_dicts"][-1].copy() if name in START else np.zeros(7, np.int64)
    for f in range(len(gts)):                                     # the dict after every frame, as the reference left it
        c, br, bo, n = R.frame_record(oracle, preds[f], gts[f], None if rois is None else rois[f], thresh)
        run += c
        assert np.array_equal(run, rz[name + "_dicts"][f]), (name, f)
        assert n == rz[name + "_ngt"][f]
        assert np.abs(br - rz[name + "_best_rcnn"][f]).max(initial=0) <= 1e-6
        assert np.abs(bo - rz[name + "_best_roi"][f]).max(initial=0) <= 1e-6


def test_golden_covers_the_quirks(rz):
    assert list(rz["plain_ngt"]) == [9, 12, 7, 6] and rz["plain_gt"].shape == (4, 12, 8)
    g = rz["plain_gt"]
    assert not g[1, 4].any() and g[1, 3].any() and g[1, 5].any()                    # an interior zero row, counted
    assert list(g[2, 7, :3]) == [1.0, -1.0, 0.0] and not g[2, 8:].any()             # a trailing row that sums to zero, trimmed
    assert rz["plain_pred_n"][3] == 0                                               # a frame without predictions
    assert not rz["plain_rois"][:, -2:].any()                                       # zero-padded RoI slots in every frame
    last = rz["plain_dicts"][-1]
    assert all(0 < v < last[0] for v in last[1:])
    assert list(rz["zero_dicts"][-1]) == [1, 0, 0, 0, 0, 0, 0] and list(rz["empty_dicts"][-1]) == [0] * 7
    assert list(rz["one_dicts"][-1][1:4]) == [0, 0, 0]
    for name in CASES:                                                              # the margin the exact-count GPU tests rely on
        for key in ("_best_rcnn", "_best_roi"):
            best = rz[name + key]
            for t in rz["thresh"]:
                assert not ((best >= 0) & (np.abs(best - t) < 1e-3)).any()


def test_trimming_rules():
    z = np.zeros((4, 8), np.float32)
    assert R.trimmed_rows(z) == 1 and R.trimmed_rows(z[:0]) == 0
    z[1, 3] = 2.0
    assert R.trimmed_rows(z) == 2
    z[3, 0], z[3, 1] = 1.0, -1.0
    assert R.trimmed_rows(z) == 2
    z[3, 7] = 1.0                                                                   # the class column is part of the sum
    assert R.trimmed_rows(z) == 4


# ---- host logic of RecallRecord ------------------------------------------------------------------------------------------

def test_record_keys_summary_and_load_counts():
    from cpd_amd.recall import RecallRecord, record_keys
    for written in ([0.3, 0.5, 0.7], [0.30, 0.50, 0.70]):                           # str(0.30) == '0.3', as the reference formats it
        rec = RecallRecord(written, device="cpu")
        assert rec.keys == record_keys(written) == ["gt", "roi_0.3", "roi_0.5", "roi_0.7", "rcnn_0.3", "rcnn_0.5", "rcnn_0.7"]
        d = rec.as_dict()
        assert d == dict.fromkeys(rec.keys, 0) and all(type(v) is int for v in d.values())
        assert rec.summary() == {"recall/roi_%s" % t: 0.0 for t in ("0.3", "0.5", "0.7")} | {"recall/rcnn_%s" % t: 0.0 for t in ("0.3", "0.5", "0.7")}
    rec.load_counts([40, 30, 20, 10, 36, 28, 4])
    assert rec.as_dict() == {"gt": 40, "roi_0.3": 30, "roi_0.5": 20, "roi_0.7": 10, "rcnn_0.3": 36, "rcnn_0.5": 28, "rcnn_0.7": 4}
    assert list(rec.as_dict()) == ["gt", "roi_0.3", "rcnn_0.3", "roi_0.5", "rcnn_0.5", "roi_0.7", "rcnn_0.7"]     # the reference's insertion order
    s = rec.summary()
    assert list(s) == ["recall/roi_0.3", "recall/rcnn_0.3", "recall/roi_0.5", "recall/rcnn_0.5", "recall/roi_0.7", "recall/rcnn_0.7"]
    assert s["recall/roi_0.3"] == 30 / 40 and s["recall/rcnn_0.7"] == 4 / 40
    rec.load_counts({"gt": 0, "roi_0.3": 0, "roi_0.5": 0, "roi_0.7": 0, "rcnn_0.3": 0, "rcnn_0.5": 0, "rcnn_0.7": 0})
    assert rec.summary()["recall/rcnn_0.5"] == 0.0                                  # max(gt, 1)
    assert RecallRecord([0.5], device="cpu").keys == ["gt", "roi_0.5", "rcnn_0.5"]
    with pytest.raises(ValueError):
        RecallRecord([], device="cpu")
    with pytest.raises(ValueError):
        RecallRecord([0.1] * 9, device="cpu")
    assert rec.reduce_() is rec                                                     # no process group: a no-op


def test_pad_gt():
    from cpd_amd.recall import pad_gt
    a, b = np.arange(16, dtype=np.float32).reshape(2, 8), np.ones((5, 8), np.float32)
    blk = pad_gt([a, np.zeros((0, 8), np.float32), b])
    assert tuple(blk.shape) == (3, 5, 8) and blk.dtype.is_floating_point
    assert np.array_equal(blk[0, :2].numpy(), a) and not blk[0, 2:].any() and not blk[1].any() and np.array_equal(blk[2].numpy(), b)
    assert tuple(pad_gt([np.zeros((0, 8), np.float32)]).shape) == (1, 0, 8)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from cpd_amd import dist_utils as du
    from cpd_amd.recall import RecallRecord
    assert du.init("gloo")
    rec = RecallRecord([0.3, 0.5, 0.7], device="cpu").load_counts([10 + rank, 7, 5, 3 * rank, 9, 6 + rank, 1])
    rec.reduce_()
    q.put((rank, rec.as_dict()))
    du.barrier()
    du.shutdown()


def test_reduce_sums_the_counters_over_two_gloo_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    out = sorted(q.get(timeout=120) for _ in range(2))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    want = {"gt": 21, "roi_0.3": 14, "roi_0.5": 10, "roi_0.7": 3, "rcnn_0.3": 18, "rcnn_0.5": 13, "rcnn_0.7": 2}
    assert out[0][1] == out[1][1] == want
