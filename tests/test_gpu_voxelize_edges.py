"""The first-appearance voxelizer at its edges (scenes: tests/ref_voxelize_edges.py; that each scene holds its edge:
tests/test_voxelize_edges_ref.py). Every scene goes through (a) cpd_voxelize (ops.Voxelizer.__call__) and (b) the batched entry point
with that one frame (ops.Voxelizer.batch([cloud])): each against the serial CPU oracle -- coordinates, row order, counts and payload
bit-exact, fused means <= 1e-6 -- and (a) against (b) bit for bit, means included. A raw cpd_voxelize call with sentinels behind
n_voxels[0], behind every output's capacity and behind the workspace shows that the one-frame entry point writes nothing there."""
import numpy as np
import pytest
import torch

import ref_voxelize_edges as R
from cpd_amd import ops

pytestmark = pytest.mark.gpu

_WANT = {}


def want(oracle, name):
    """the oracle's rows of a scene, computed once: (scene, voxels, coords, num_points, means)"""
    if name not in _WANT:
        sc = R.SCENES[name]()
        v0, c0, n0 = oracle.voxelize(sc["points"], sc["voxel_size"], sc["point_cloud_range"], sc["P"], sc["max_voxels"])
        m0 = oracle.mean_vfe(v0, n0) if len(n0) else np.zeros((0, sc["points"].shape[1]), np.float32)
        for a in (v0, c0, n0, m0):
            a.setflags(write=False)
        _WANT[name] = (sc, v0, c0, n0, m0)
    return _WANT[name]


def voxelizer(sc):
    return ops.Voxelizer(sc["voxel_size"], sc["point_cloud_range"], sc["points"].shape[1], sc["P"], sc["max_voxels"])


def against_oracle(got, w, batch_idx, what):
    v, c, n, mean = [t.cpu().numpy() for t in got]
    sc, v0, c0, n0, m0 = w
    assert len(c) == len(c0), what
    np.testing.assert_array_equal(c[:, -3:], c0, err_msg=what)
    if c.shape[1] == 4:
        assert (c[:, 0] == batch_idx).all(), what
    np.testing.assert_array_equal(n, n0, err_msg=what)
    np.testing.assert_array_equal(v, v0, err_msg=what)
    np.testing.assert_allclose(mean, m0, rtol=1e-6, atol=1e-6, err_msg=what)


def one_frame_and_batch(oracle, name, coord_cols=4, batch_idx=0):
    w = want(oracle, name)
    sc = w[0]
    pts = torch.from_numpy(sc["points"]).cuda()
    vox = voxelizer(sc)
    a = vox(pts, batch_idx=batch_idx, coord_cols=coord_cols, want_voxels=True, want_mean=True, sync=True)
    assert a[4] == len(w[2]), name
    against_oracle(a[:4], w, batch_idx, name + " cpd_voxelize")
    vb, cb, nb, mb, nvox = vox.batch([pts], want_voxels=True)
    k = nvox.cpu().numpy()
    assert k.shape == (2,) and k[0] == k[1] == a[4], name
    b = [t[:k[0]] for t in (vb, cb, nb, mb)]
    against_oracle(b, w, 0, name + " cpd_voxelize_batch_frames")
    assert torch.equal(a[1][:, -3:], b[1][:, 1:]) and torch.equal(a[2], b[2]), name
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]), name                   # the means too: the same kernels' sums


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_scene_one_frame_and_batch_of_one(oracle, hip, name):
    one_frame_and_batch(oracle, name)


@pytest.mark.parametrize("coord_cols,batch_idx", R.COORD_PARAMS)
def test_coord_columns_and_batch_index(oracle, hip, coord_cols, batch_idx):
    one_frame_and_batch(oracle, "c5", coord_cols, batch_idx)
    one_frame_and_batch(oracle, "late_voxels_cap", coord_cols, batch_idx)


SENT_I, SENT_F, PAD = -77777, -12345.5, 7


@pytest.mark.parametrize("name", R.RAW_SCENES)
@pytest.mark.parametrize("coord_cols", [3, 4])
def test_raw_call_writes_one_count_and_nothing_behind_the_capacity(oracle, hip, name, coord_cols):
    """cpd_voxelize's n_voxels is ONE int and its outputs hold min(max_voxels, n_points) rows: the ints behind n_voxels[0], PAD rows
    behind every output and the bytes behind the workspace's queried size keep their sentinels (rows between the count and the
    capacity are unspecified and not looked at)."""
    from cpd_amd._lib import check, farr, lib, ptr, stream
    sc, v0, c0, n0, m0 = want(oracle, name)
    pts = torch.from_numpy(sc["points"]).cuda()
    n, c = pts.shape
    P, maxv, vs, rg = sc["P"], sc["max_voxels"], sc["voxel_size"], sc["point_cloud_range"]
    cap = min(maxv, n)
    assert (n == 0) == (name == "no_points") and (cap == maxv) == (name == "late_voxels_cap")
    voxels = torch.full((cap + PAD, P, c), SENT_F, device="cuda")
    coords = torch.full((cap + PAD, coord_cols), SENT_I, dtype=torch.int32, device="cuda")
    num = torch.full((cap + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    mean = torch.full((cap + PAD, c), SENT_F, device="cuda")
    nvox = torch.full((4,), SENT_I, dtype=torch.int32, device="cuda")
    nbytes = lib().cpd_voxelize_workspace_bytes(n, P, maxv, farr(vs), farr(rg))
    assert nbytes > 0
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    check(lib().cpd_voxelize(ptr(pts), n, c, farr(vs), farr(rg), P, maxv, 3, coord_cols, ptr(voxels), ptr(coords), ptr(num), ptr(mean),
                             ptr(nvox), ptr(ws), nbytes, stream()), "cpd_voxelize")
    torch.cuda.synchronize()
    k = nvox.cpu().numpy()
    assert k[0] == len(c0) <= cap and (k[1:] == SENT_I).all()
    assert (coords[cap:] == SENT_I).all() and (num[cap:] == SENT_I).all()
    assert (voxels[cap:] == SENT_F).all() and (mean[cap:] == SENT_F).all()
    assert (ws[nbytes:] == 0xA5).all()
    against_oracle([t[:k[0]] for t in (voxels, coords, num, mean)], (sc, v0, c0, n0, m0), 3, name)
