"""GPU checks of the OYSTER generator (cpd_amd.oyster, csrc/oyster.hip): cpd_oyster_align_tracks against the numpy restatement
(tests/ref_oyster.py) on random and hand-built tracks, and the written file for both branches against the reference's golden
(tests/golden/oyster.npz) and against the restatement fed the GPU's own per-frame boxes.

The rule for aligned boxes (_check_aligned): l, w, h, yaw and z bit-equal; x and y within 1e-6 -- the only source of a
difference is one float32 ulp in cos / sin (device against host libm before the rounding) times an offset of at most max_len =
12 m, 12 * 2^-24 = 7e-7 -- and at most 1 % of the rows may differ in x, y by more than 1e-9."""
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_golden_oyster as MG  # noqa: E402
import ref_oyster as RO  # noqa: E402
from make_golden_mfcf import write_sequence  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ('outline_box', 'outline_ids', 'outline_cls', 'outline_dif')


@pytest.fixture(scope="module")
def O():
    from cpd_amd import oyster
    return oyster


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "oyster.npz")))


@pytest.fixture(scope="module")
def drive(gold):
    infos = MG.box_drive(int(gold["seed"]), int(gold["n_frames_b"]))
    assert MG.drive_digest(infos) == str(gold["digest_b"])
    return infos


@pytest.fixture(scope="module")
def seq_a(gold):
    frames, poses = MG.sequence_a(int(gold["seed"]))
    assert MG.digest(frames, poses) == str(gold["digest_a"])
    return frames, poses


def _check_aligned(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1, 7), np.asarray(want, np.float64).reshape(-1, 7)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got[:, 2:].view(np.uint64), want[:, 2:].view(np.uint64))      # z l w h yaw: the same bits
    if len(want) == 0:
        return
    err = np.abs(got[:, 0:2] - want[:, 0:2]).max(1)
    print("x, y: worst %.3g, %d of %d rows past 1e-9" % (err.max(), int((err > 1e-9).sum()), len(err)))
    assert err.max() <= 1e-6
    assert (err > 1e-9).sum() <= 0.01 * len(err)


def _check_infos(got, want):
    """The file rule: the same frames, ids, classes and dif equal, boxes under the rule above (over the whole file)."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in KEYS:
            assert np.asarray(g[k]).shape == np.asarray(w[k]).shape and np.asarray(g[k]).dtype == np.asarray(w[k]).dtype, (i, k)
        for k in KEYS[1:]:
            np.testing.assert_array_equal(g[k], w[k])
    _check_aligned(np.concatenate([g['outline_box'] for g in got]), np.concatenate([w['outline_box'] for w in want]))


def _random_tracks(rng, lengths):
    n = int(np.sum(lengths))
    ang, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(2, 70, n)
    boxes = np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(-1, 3, n), rng.uniform(0.3, 12, n), rng.uniform(0.3, 3, n),
                      rng.uniform(0.5, 4, n), rng.uniform(-2 * np.pi, 2 * np.pi, n)], 1)
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(lengths)
    return boxes, off


# ---- the kernel against the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [6, 7, 60, 79, 80, 257, 1025])      # 257: past the workgroup's width; 1025: past the LDS tile
def test_one_track(O, n):
    boxes, off = _random_tracks(np.random.default_rng(100 + n), [n])
    got = O.align_tracks(boxes, off)
    _check_aligned(got, RO.align_track(boxes))


def test_three_thousand_short_tracks(O):
    boxes, off = _random_tracks(np.random.default_rng(31), [6] * 3000)           # the grid is far past the CU count
    _check_aligned(O.align_tracks(boxes, off), RO.align_tracks(boxes, off))


def test_mixed_lengths_in_one_launch(O):
    lengths = [1025, 6, 2100, 6, 257, 7, 80, 79, 60, 6, 1025, 5200, 6]            # the longest and the shortest side by side;
    assert O.track_top(5200) > 256                                                # 5200: more ranks than one summing window
    boxes, off = _random_tracks(np.random.default_rng(32), lengths)
    _check_aligned(O.align_tracks(boxes, off), RO.align_tracks(boxes, off))
    assert set(np.concatenate([RO.align_track(boxes[a:b], return_choice=True)[1] for a, b in zip(off[:4], off[1:5])])) == {0, 1, 2, 3}


def test_ties(O):
    """Coinciding candidates (the first wins) and equal distances (the lower row sorts first)."""
    boxes, off, _ = RO.tie_tracks()
    got = O.align_tracks(boxes, off)
    _check_aligned(got, RO.align_tracks(boxes, off))
    a, b = off[2], off[3]                                            # l_off == w_off == 0: only z moves, to float32
    np.testing.assert_array_equal(got[a:b, 0:3], boxes[a:b, 0:3].astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(got[a:b, 3:], boxes[a:b, 3:])
    # eight boxes at one place with different sizes: the consensus is over rows 0, 1, 2, whatever order they sit in memory
    same = np.tile([[20.0, -10.0, 0.75, 0, 0, 1.5, 0.4]], (8, 1))
    same[:, 3], same[:, 4] = [4.0, 5.0, 6.5, 3.0, 3.1, 3.2, 3.3, 9.0], [2.0, 1.5, 2.5, 1.0, 1.1, 1.2, 1.3, 2.9]
    got = O.align_tracks(same, np.array([0, 8]))
    _check_aligned(got, RO.align_track(same))
    assert RO.consensus(same) == ((4.0 + 5.0 + 6.5) / 3, (2.0 + 1.5 + 2.5) / 3)


def test_no_tracks(O):
    import torch
    from cpd_amd import _lib
    assert O.align_tracks(np.zeros((0, 7)), np.array([0])).shape == (0, 7)
    lib = _lib.lib()
    d = torch.zeros((4, 7), dtype=torch.float64, device="cuda")
    off = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((4, 7), 7.0, dtype=torch.float64, device="cuda")
    assert lib.cpd_oyster_align_tracks(_lib.ptr(d), _lib.ptr(off), _lib.ptr(off), 0, 4, _lib.ptr(out), _lib.stream()) == 0
    assert lib.cpd_oyster_align_tracks(_lib.ptr(d), None, _lib.ptr(off), 1, 4, _lib.ptr(out), _lib.stream()) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    # empty tracks between full ones write nothing of their own
    boxes, _ = _random_tracks(np.random.default_rng(33), [6, 7])
    off = np.array([0, 0, 6, 6, 6, 13, 13])
    _check_aligned(O.align_tracks(boxes, off), RO.align_tracks(boxes, off))


# ---- run B: the box branch, end to end -------------------------------------------------------------------------------------------

def test_run_b_end_to_end(O, gold, drive, tmp_path, monkeypatch):
    root = str(tmp_path)
    MG.write_box_drive(root, drive)
    monkeypatch.setattr(O.outline.OutlineGPU, "frames_boxes",
                        lambda *a, **k: pytest.fail("every frame carries boxes: the per-frame chain must not run"))
    launches = []
    real = O.launch_align
    monkeypatch.setattr(O, "launch_align", lambda *a: launches.append(int(a[2].shape[0])) or real(*a))
    want = MG.unpack_infos(gold, "finb", len(drive))
    infos = O.OYSTER(MG.SEQ_B, root, MG.config_b())()
    _check_infos(infos, want)
    assert all(np.array_equal(i['pose'], d['pose']) for i, d in zip(infos, drive))
    out_pkl = os.path.join(root, MG.SEQ_B, MG.SEQ_B + "_outline_OYSTER.pkl")
    with open(out_pkl, "rb") as f:
        _check_infos(pickle.load(f), want)
    # no cache: a second run computes again and overwrites what it finds
    with open(out_pkl, "wb") as f:
        pickle.dump([dict(marker="stale")], f)
    again = O.OYSTER(MG.SEQ_B, root, MG.config_b())()
    with open(out_pkl, "rb") as f:
        written = pickle.load(f)
    for g, w, first in zip(again, written, infos):
        for k in KEYS:
            np.testing.assert_array_equal(g[k], w[k])
            np.testing.assert_array_equal(g[k], first[k])
    kept = sum(1 for n in gold["lengths_b"] if n >= 6)
    assert launches == [kept, kept]                                  # one launch per run, over all kept tracks


# ---- run A: the point branch, end to end -----------------------------------------------------------------------------------------

def test_run_a_end_to_end(O, gold, seq_a, tmp_path):
    frames, poses = seq_a
    root = str(tmp_path)
    write_sequence(root, frames, poses, seq=MG.SEQ_A)
    cfg = MG.config_a()
    gen = O.OYSTER(MG.SEQ_A, root, cfg, chunk=5)                      # four chunks, the last one short, both dtypes in each
    boxes, got_poses = gen.per_frame_boxes([dict(pose=p) for p in poses])
    n_box = n_flag = 0
    for i in range(len(frames)):
        ref, flag = gold["pfa%d_box" % i], gold["pfa%d_flag" % i]
        b = np.asarray(boxes[i], np.float64).reshape(-1, 7)
        assert b.shape == ref.shape, "frame %d" % i
        np.testing.assert_allclose(b[~flag], ref[~flag], rtol=0, atol=1e-9)
        n_box, n_flag = n_box + len(ref), n_flag + int(flag.sum())
    assert n_box >= 40 and n_flag <= 0.10 * n_box
    # a differing hull legitimately changes the tracker's output: the file is compared with the composition (the GPU's own
    # per-frame boxes through the host restatement), not with the golden's final infos
    want = RO.generate(boxes, poses, cfg["GeneratorConfig"])
    infos = gen()
    assert sum(len(w['outline_ids']) for w in want) >= 40
    _check_infos(infos, want)
    with open(os.path.join(root, MG.SEQ_A, MG.SEQ_A + "_outline_OYSTER.pkl"), "rb") as f:
        _check_infos(pickle.load(f), want)


def test_create_oyster_equals_single_runs(O, seq_a, drive, tmp_path):
    frames, poses = seq_a
    cfg = MG.config_a()
    for root in (str(tmp_path / "a"), str(tmp_path / "b")):
        write_sequence(root, frames, poses, seq=MG.SEQ_A)
        MG.write_box_drive(root, drive)
    both = O.create_oyster([MG.SEQ_A, MG.SEQ_B], str(tmp_path / "a"), cfg, chunk=7)
    singles = [O.OYSTER(s, str(tmp_path / "b"), cfg)() for s in (MG.SEQ_A, MG.SEQ_B)]
    for got, want, n in zip(both, singles, (len(frames), len(drive))):
        assert len(got) == len(want) == n
        for g, w in zip(got, want):
            for k in KEYS:
                np.testing.assert_array_equal(g[k], w[k])
    assert sum(len(g['outline_ids']) for g in both[0]) >= 40 and sum(len(g['outline_ids']) for g in both[1]) >= 300


def test_mixed_frames_take_both_branches(O, gold, seq_a, tmp_path, monkeypatch):
    """Every third frame carries the reference's boxes in its info; the others are read and go through the chain."""
    frames, poses = seq_a
    root, seq, cfg = str(tmp_path), "segment-97531864_oyster", MG.config_a()
    carried = [i for i in range(len(frames)) if i % 3 == 0]
    write_sequence(root, frames, poses, seq=seq)
    for i in carried:
        os.remove(os.path.join(root, seq, "%04d.npy" % i))           # a frame that brings its boxes is never read
    with open(os.path.join(root, seq, seq + ".pkl"), "wb") as f:
        pickle.dump([dict(pose=p.copy(), **(dict(outline_box=np.array(gold["pfa%d_box" % i])) if i in carried else {}))
                     for i, p in enumerate(poses)], f)
    seen = []
    real = O.outline.OutlineGPU.frames_boxes

    def counting(self, batch):
        seen.append(len(batch))
        return real(self, batch)

    monkeypatch.setattr(O.outline.OutlineGPU, "frames_boxes", counting)
    gen = O.OYSTER(seq, root, cfg, chunk=4)
    infos = gen()
    assert sum(seen) == len(frames) - len(carried) and max(seen) <= 4
    with open(os.path.join(root, seq, seq + ".pkl"), "rb") as f:
        chain, _ = gen.per_frame_boxes(pickle.load(f))               # the same composition once more, for the host restatement
    for i in carried:
        np.testing.assert_array_equal(chain[i], gold["pfa%d_box" % i])
    _check_infos(infos, RO.generate(chain, poses, cfg["GeneratorConfig"]))
