"""GPU: cpd_amd.ppscore (csrc/ppscore.hip) against the reference's recorded counts and float16 H (tests/golden/ppscore.npz),
and against the numpy restatement (tests/ref_ppscore.py) and literal counts on hand-built cases."""
import os
import pickle
import warnings

import numpy as np
import pytest

import ref_ppscore as R
from test_ppscore_ref import check_h, golden_run, golden_sequence

pytestmark = pytest.mark.gpu
S = 1.0 / 16     # hand-built coordinates sit on this grid: every difference and square is exact


@pytest.fixture(scope="module")
def P(hip):
    from cpd_amd import ppscore
    return ppscore


@pytest.fixture(scope="module")
def G(P):
    return P.PPScoreGPU()


@pytest.fixture(scope="module")
def pz(golden):
    return golden("ppscore")


def run(G, query, travs, r, poses=None, inv=None):
    c, h = G.run(G.upload(query), [G.upload(t) for t in travs], poses, inv, r)
    return c.cpu().numpy().astype(np.int64), h.cpu().numpy()


def pts(rows, dtype=np.float32):
    a = np.asarray(rows, np.float64).reshape(-1, 3)
    out = a.astype(dtype)
    assert np.array_equal(out.astype(np.float64), a)     # representable: the case is what it says
    return out


# ---- 1. golden ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,run_name", [("A", "w6"), ("A", "def"), ("B", "w6"), ("B", "def")])
def test_golden_counts_and_h(G, pz, name, run_name):
    frames, poses = golden_sequence(pz, name)
    gold, (max_win, win_inte) = golden_run(pz, name, run_name)
    dev = [G.upload(f) for f in frames]      # [N, 5] float16 rows: the kernel reads with the row stride
    for i in range(len(frames)):
        js = R.window(i, len(frames), max_win, win_inte)
        c, h = G.run(dev[i], [dev[j] for j in js], [poses[j] for j in js], np.linalg.inv(poses[i]), 0.3)
        np.testing.assert_array_equal(c.cpu().numpy(), gold[i][0], err_msg="%s %s frame %d" % (name, run_name, i))
        check_h(h.cpu().numpy(), gold[i][1], gold[i][2], "%s %s frame %d" % (name, run_name, i))


# ---- 2. hand-built exactness ------------------------------------------------------------------------------------------------

def exact_cases():
    cases = {}
    far = 2.0 ** 17        # 2^18 cells of side 0.5: the clump there aliases with the one at x = 1
    axis = [[s * k * S if a == ax else 0.0 for a in range(3)] for ax in range(3) for s in (1, -1) for k in (1, 7, 8, 9)]
    q = pts([[1, 1, 1], [0, 0, 0], [-S, 0, 0], [40, 40, 40], [1 + far, 1, 1]])
    t0 = pts([[1.5, 1, 1], [1, 1.5, 1], [1, 1, 0.5], [1.5625, 1, 1]]      # d == r three times, one step beyond once
             + axis                                                      # either side of the cell faces, negative cells
             + [[1, 1, 1]] * 3                                           # duplicates of the query
             + [[1 + far, 1, 1]] * 2 + [[1.25 + far, 1, 1]])
    t2 = pts([[1, 1, 1.25]])
    cases["r05_faces_duplicates_alias_empty"] = (q, [t0, pts([]), t2], 0.5,
                                                 [[6, 0, 1], [18, 0, 0], [14, 0, 0], [0, 0, 0], [3, 0, 0]])
    cases["r03_half"] = (pts([[2, 2, 2]], np.float16),
                         [pts([[2.25, 2, 2], [2.3125, 2, 2], [2, 1.75, 2], [2, 2, 2.3125]], np.float16), pts([[2, 2, 2]], np.float16)],
                         0.3, [[2, 1]])
    cases["r0625_pythagorean"] = (pts([[0, 0, 0]]), [pts([[6 * S, 8 * S, 0], [6 * S, 8 * S, S]]), pts([[-8 * S, 0, -6 * S]])],
                                  0.625, [[1, 1]])
    cases["no_query"] = (pts([]), [pts([[0, 0, 0]]), pts([[1, 0, 0]])], 0.5, np.zeros((0, 2), np.int64))
    return cases


@pytest.mark.parametrize("case", sorted(exact_cases()))
def test_exact_counts(G, case):
    q, travs, r, want = exact_cases()[case]
    c, h = run(G, q, travs, r)
    np.testing.assert_array_equal(c, np.asarray(want, np.int64).reshape(len(q), len(travs)))
    np.testing.assert_array_equal(c, R.count_neighbors(q, travs, r))
    np.testing.assert_array_equal(h.view(np.uint16), R.ephe_score(c).astype(np.float16).view(np.uint16))
    if case.startswith("r05"):
        assert h.view(np.uint16)[3] == 0         # no neighbour anywhere: the row is zero and H == +0
        assert c[0, 1] == 0 and c[:, 1].sum() == 0


# ---- 3. dense cell ----------------------------------------------------------------------------------------------------------

def test_dense_cell(G):
    rng = np.random.default_rng(4)
    d = rng.normal(size=(20000, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.249 * rng.random((20000, 1)) ** (1 / 3))
    cloud = (np.array([5.0, 5.0, 5.0]) + d).astype(np.float32)
    assert np.linalg.norm(cloud.astype(np.float64) - 5.0, axis=1).max() < 0.25
    c, _ = run(G, pts([[5, 5, 5]]), [cloud, pts([[9, 9, 9]])], 0.3)
    np.testing.assert_array_equal(c, [[20000, 0]])


# ---- 4. poses ---------------------------------------------------------------------------------------------------------------

def test_poses_exact(G):
    def pose(rot, t):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = rot, t
        return m
    rz90, rz180 = [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]
    rx270 = [[1, 0, 0], [0, 0, 1], [0, -1, 0]]
    cur = pose(rz90, [10, -20, 3])
    tp = [pose(rz180, [7, 5, 1]), pose(rx270, [-300, 40, 0]), cur]
    # where the traversal points are to land in the current frame, and the literal counts for the query (1, 1, 1), r = 0.5
    land = [pts([[1.5, 1, 1], [1, 1, 1.5625], [1, 1, 1]]), pts([[1, 0.5, 1]]), pts([[1, 1, 1.5], [1.0625, 1, 1], [3, 1, 1]])]
    travs = []
    for m, d in zip(tp, land):
        w = (np.linalg.inv(m) @ cur @ np.concatenate([d.astype(np.float64), np.ones((len(d), 1))], 1).T).T[:, :3]
        travs.append(pts(w))
    inv = np.linalg.inv(cur)
    for m, t, d in zip(tp, travs, land):
        np.testing.assert_array_equal(R.rigid(R.rigid(t, m), inv), d)      # every product is exact in any order
    q = pts([[1, 1, 1]])
    c, h = run(G, q, travs, 0.5, tp, inv)
    np.testing.assert_array_equal(c, [[2, 1, 2]])
    np.testing.assert_array_equal(c, R.count_neighbors(q, land, 0.5))
    np.testing.assert_array_equal(h.view(np.uint16), R.ephe_score(c).astype(np.float16).view(np.uint16))


# ---- 5. order independence and repeatability ----------------------------------------------------------------------------------

def test_order_independence(G):
    rng = np.random.default_rng(8)
    q = np.concatenate([rng.uniform(-3, 3, (3001, 3)), rng.uniform(0, 1, (3001, 2))], 1).astype(np.float16)
    travs = [rng.uniform(-3, 3, (n, 3)).astype(np.float16) for n in (2500, 1777, 3100, 64, 2900)]
    c0, h0 = run(G, q, travs, 0.3)
    assert 0 < (c0 == 0).mean() < 1 and c0.max() > 3
    np.testing.assert_array_equal(c0, R.count_neighbors(q, travs, 0.3))
    c1, h1 = run(G, q, travs, 0.3)
    assert np.array_equal(c0, c1) and np.array_equal(h0.view(np.uint16), h1.view(np.uint16))
    perm = rng.permutation(len(q))
    c2, h2 = run(G, q[perm], travs, 0.3)
    assert np.array_equal(c2, c0[perm]) and np.array_equal(h2.view(np.uint16), h0.view(np.uint16)[perm])
    c3, h3 = run(G, q, [t[rng.permutation(len(t))] for t in travs], 0.3)
    assert np.array_equal(c3, c0) and np.array_equal(h3.view(np.uint16), h0.view(np.uint16))
    tperm = [3, 0, 4, 2, 1]
    c4, h4 = run(G, q, [travs[t] for t in tperm], 0.3)
    assert np.array_equal(c4, c0[:, tperm])
    assert R.half_steps(h4, h0).max() <= 1      # the sum over traversals is reordered


# ---- 6. fewer than two traversals ---------------------------------------------------------------------------------------------

def write_sequence(root, seq, frames, poses):
    os.makedirs(os.path.join(root, seq))
    for i, f in enumerate(frames):
        np.save(os.path.join(root, seq, "%04d.npy" % i), f)
    with open(os.path.join(root, seq, seq + ".pkl"), "wb") as f:
        pickle.dump([{"pose": p} for p in poses], f)


def test_single_traversal_is_nan(G, P, pz, tmp_path):
    frames, poses = golden_sequence(pz, "A")
    c, h = run(G, frames[0], [frames[0]], 0.3)
    assert c.shape == (len(frames[0]), 1) and c.min() >= 1 and np.isnan(h).all()
    write_sequence(str(tmp_path), "one", frames[:1], poses[:1])
    with pytest.warns(UserWarning, match="fewer than two traversals"):
        assert P.save_pp_score("one", str(tmp_path)) is True
    got = np.load(os.path.join(str(tmp_path), "one", "ppscore", "0000.npy"))
    assert got.dtype == np.float16 and got.shape == (len(frames[0]),) and np.isnan(got).all()


# ---- 7. driver ----------------------------------------------------------------------------------------------------------------

def check_files(pz, root, seq, run_name):
    gold, _ = golden_run(pz, "A", run_name)
    out_dir = os.path.join(root, seq, "ppscore")
    assert sorted(os.listdir(out_dir)) == ["%04d.npy" % i for i in range(len(gold))]
    for i, (_, h, tie) in enumerate(gold):
        got = np.load(os.path.join(out_dir, "%04d.npy" % i))
        check_h(got, h, tie, "%s frame %d" % (run_name, i))
        np.testing.assert_array_equal((got > 0.7)[~tie], (h > 0.7)[~tie])      # MFCF's selection (ppscore_thresh 0.7)


def test_driver(P, pz, tmp_path):
    frames, poses = golden_sequence(pz, "A")
    root = str(tmp_path)
    for seq in ("segment-a", "segment-b"):
        write_sequence(root, seq, frames, poses)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*fewer than two traversals.*")
        assert P.save_pp_score("segment-a", root, 6, 1) is True
        check_files(pz, root, "segment-a", "w6")
        assert P.save_pp_score("segment-a", root) is True        # recomputes and overwrites
        check_files(pz, root, "segment-a", "def")
        assert P.create_ppscore(["segment-a", "segment-b"], root, 6, 1) == [True, True]
    for seq in ("segment-a", "segment-b"):
        check_files(pz, root, seq, "w6")
    os.remove(os.path.join(root, "segment-b", "0003.npy"))
    with pytest.raises(FileNotFoundError):
        P.save_pp_score("segment-b", root, 6, 1)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------

def test_error_codes(G, P, hip):
    import ctypes
    import torch
    from cpd_amd import _lib
    lib = _lib.lib()
    q = pts([[0, 0, 0], [1, 0, 0]])
    t = pts([[0, 0, 0.25]])
    with pytest.raises(_lib.CpdHipError, match="UNSUPPORTED"):
        run(G, q, [t] * 17, 0.3)
    for r in (0.0, -0.3, float("nan")):
        with pytest.raises(_lib.CpdHipError, match="CPD_ERR_ARG"):
            run(G, q, [t, t], r)
    with pytest.raises(TypeError):
        P.count_neighbors(q.astype(np.float64), [t])
    with pytest.raises(TypeError):
        P.compute_ppscore(q, [t, t.astype(np.float64)])
    dq, dt = G.upload(q), G.upload(np.concatenate([t, t]))
    off = (ctypes.c_int32 * 18)(0, 1, 2)
    nb = lib.cpd_ppscore_workspace_bytes(2, 2, 2)
    ws = torch.empty(nb, dtype=torch.uint8, device=G.device)
    cnt = torch.empty(4, dtype=torch.int32, device=G.device)
    args = lambda n_trav, nbytes: (_lib.ptr(dq), 2, 3, 0, _lib.ptr(dt), off, n_trav, 3, 0, None, None, 0.3, _lib.ptr(cnt), None,
                                   _lib.ptr(ws), nbytes, _lib.stream())
    assert lib.cpd_ppscore(*args(17, nb)) == -4
    assert lib.cpd_ppscore(*args(2, nb - 1)) == -2
    assert lib.cpd_ppscore(*args(2, nb)) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cnt.cpu().numpy().reshape(2, 2), [[1, 1], [0, 0]])
    # the module's surface: count_neighbors takes a dict in its order, compute_ppscore returns float64 H
    c = P.count_neighbors(q, {"a": t, "b": pts([[1, 0, 0], [1, 0, 0.5]])}, 0.5)
    assert c.dtype == np.int64
    np.testing.assert_array_equal(c, [[1, 0], [0, 2]])
    H = P.compute_ppscore(q, [t, pts([[1, 0, 0], [1, 0, 0.5]])], 0.5)
    assert H.dtype == np.float64
    np.testing.assert_allclose(H, R.ephe_score(c), rtol=1e-15, atol=0)
    m = np.eye(4)
    m[:3, 3] = [5000.0, 2500.0, 1.0]
    np.testing.assert_array_equal(P.points_rigid_transform(q, m), R.rigid(q, m))
