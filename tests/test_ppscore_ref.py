"""CPU: the numpy restatement of the PP-score precompute (tests/ref_ppscore.py) against the reference's recorded output
(tests/golden/ppscore.npz, written by make_golden_ppscore.py), the synthetic sequence, and the new C-ABI entry points'
host-side behaviour (no kernel is launched)."""
import ctypes
import hashlib
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import ref_ppscore as R
from cpd_amd.synthetic import ppscore_sequence

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pz(golden):
    return golden("ppscore")


_SEQ_CACHE = {}


def golden_sequence(pz, name):
    """(frames, poses) of golden sequence `name`, regenerated from its seed and checked against the stored digest."""
    if name not in _SEQ_CACHE:
        frames, poses = ppscore_sequence(int(pz[name + "_seed"]), int(pz["n_frames"]), int(pz["n_az"]), np.float16,
                                         tuple(pz[name + "_origin"]))
        h = hashlib.sha256()
        for f, p in zip(frames, poses):
            h.update(np.ascontiguousarray(f).tobytes())
            h.update(np.ascontiguousarray(p).tobytes())
        assert h.hexdigest() == str(pz[name + "_digest"]), (
            "ppscore_sequence(%d) no longer reproduces the golden's input (numpy RNG or synthetic.py changed): regenerate "
            "tests/golden/ppscore.npz" % int(pz[name + "_seed"]))
        assert [len(f) for f in frames] == pz[name + "_n"].tolist()
        _SEQ_CACHE[name] = (frames, poses)
    return _SEQ_CACHE[name]


def golden_run(pz, name, run):
    """Per frame (counts [N, T] int64, h [N] float16, tie [N] bool) of the reference, and the run's (max_win, win_inte)."""
    p = "%s_%s_" % (name, run)
    n, T = pz[name + "_n"], pz[p + "T"]
    counts, h = pz[p + "counts"], pz[p + "h"]
    tie = np.unpackbits(pz[p + "tie"])[:int(n.sum())].astype(bool)
    out, oc, oh = [], 0, 0
    for ni, ti in zip(n, T):
        out.append((counts[oc:oc + ni * ti].reshape(ti, ni).T.astype(np.int64), h[oh:oh + ni], tie[oh:oh + ni]))
        oc += ni * ti
        oh += ni
    args = pz["run_args"][list(pz["runs"]).index(run)]
    return out, (int(args[0]), int(args[1]))


def check_h(got, want, tie, what=""):
    """Rule 1 of the golden: float16 bits equal outside the tie mask, within one float16 step inside it."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float16 and got.shape == want.shape, what
    steps = R.half_steps(got, want)
    assert np.array_equal(got.view(np.uint16)[~tie], want.view(np.uint16)[~tie]), "%s: %d points differ outside the tie mask" % (
        what, int((got.view(np.uint16)[~tie] != want.view(np.uint16)[~tie]).sum()))
    assert steps.max(initial=0) <= 1, what


def test_fma_emulation_is_correctly_rounded():
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=4000), rng.normal(size=4000)
    c = np.where(rng.random(4000) < 0.5, -a * b * (1 + rng.normal(size=4000) * 1e-15), rng.normal(size=4000))   # half cancel
    got = R.fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    assert (got != a * b + c).any()     # the inputs do tell a fused from an unfused product


def test_golden_discriminates(pz):
    for name in pz["seqs"]:
        runs, _ = golden_run(pz, str(name), "w6")
        assert sum(c.shape[1] == 12 for c, _, _ in runs) >= 2
        for c, h, tie in runs:
            assert tie.mean() < 1e-3
            if c.shape[1] == 12:
                assert 0.05 < (h.astype(np.float64) > 0.7).mean() < 0.95
        runs, args = golden_run(pz, str(name), "def")
        assert args == (30, 5) and max(c.shape[1] for c, _, _ in runs) <= 3


@pytest.mark.parametrize("name,run,frames_checked", [("A", "w6", (0, 7, 13)), ("B", "w6", (6,)), ("A", "def", (4,)),
                                                     ("B", "def", (0, 9))])
def test_restatement_matches_reference(pz, name, run, frames_checked):
    frames, poses = golden_sequence(pz, name)
    gold, (max_win, win_inte) = golden_run(pz, name, run)
    for i in frames_checked:
        trav = R.frame_traversals(frames, poses, i, max_win, win_inte)
        c = R.count_neighbors(frames[i][:, 0:3], trav, 0.3)
        np.testing.assert_array_equal(c, gold[i][0])
        np.testing.assert_array_equal(R.ephe_score(c).astype(np.float16).view(np.uint16), gold[i][1].view(np.uint16))


def test_restatement_counts_against_brute_force():
    rng = np.random.default_rng(9)
    q = (rng.integers(-40, 40, (300, 3)) / 16).astype(np.float32)
    p = (rng.integers(-40, 40, (500, 3)) / 16).astype(np.float32)
    for r in (0.5, 0.3):
        d = q[:, None, :].astype(np.float64) - p[None].astype(np.float64)
        want = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= r * r).sum(1)
        np.testing.assert_array_equal(R.count_one(q, p, r), want)


def test_sequence_generator():
    frames, poses = ppscore_sequence(5, 3, 40, np.float32, origin=(100.0, -50.0, 2.0))
    f0, p0 = ppscore_sequence(5, 3, 40, np.float32)
    assert len(frames) == len(poses) == 3
    for f, g, p, q in zip(frames, f0, poses, p0):
        assert f.dtype == np.float32 and f.ndim == 2 and f.shape[1] == 5 and len(f) > 1000
        assert np.array_equal(f, g)             # the origin moves the poses, not the sweeps
        assert p.dtype == np.float64 and p.shape == (4, 4)
        np.testing.assert_array_equal(p[:3, 3] - q[:3, 3], [100.0, -50.0, 2.0])
        np.testing.assert_allclose(p[:3, :3] @ p[:3, :3].T, np.eye(3), atol=1e-15)
    assert not np.array_equal(poses[0], poses[1])
    with pytest.raises(TypeError):
        ppscore_sequence(5, 1, 40, np.float64)


def test_abi_entry_points_and_error_codes():
    from cpd_amd import _lib
    lib = _lib.lib()
    for name in ("cpd_ppscore_workspace_bytes", "cpd_ppscore"):          # (argument types: test_abi checks every row of the table)
        assert hasattr(lib, name)
    assert _lib.SIGNATURES["cpd_ppscore"][0] is ctypes.c_int and _lib.SIGNATURES["cpd_ppscore_workspace_bytes"][0] is ctypes.c_size_t
    nb = lib.cpd_ppscore_workspace_bytes(1000, 12000, 12)
    assert nb >= 2 * 12000 * 8 + 12000 * 16 + 1000 * 12 * 4     # table keys, members, counts
    assert lib.cpd_ppscore_workspace_bytes(0, 0, 2) > 0
    off = (ctypes.c_int32 * 18)(*([0] * 18))
    ws = ctypes.create_string_buffer(int(lib.cpd_ppscore_workspace_bytes(0, 0, 2)))
    wsp = ctypes.cast(ws, ctypes.c_void_p)

    def call(n_trav=2, radius=0.3, ws_bytes=len(ws), strides=(3, 3), dtypes=(0, 0)):
        return lib.cpd_ppscore(None, 0, strides[0], dtypes[0], None, off, n_trav, strides[1], dtypes[1], None, None, radius, None,
                               None, wsp, ws_bytes, None)

    assert call() == 0                                    # n_query == 0 is legal (and launches nothing)
    assert call(n_trav=17) == -4
    assert call(radius=0.0) == call(radius=-1.0) == call(radius=float("nan")) == -1
    assert call(ws_bytes=16) == -2
    assert call(strides=(2, 3)) == call(dtypes=(0, 2)) == -1
