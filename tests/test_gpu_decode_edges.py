"""cpd_center_decode on tied, saturated and degenerate heat maps, against the oracle (fixtures: tests/ref_decode_edges.py).

topk_class_kernel has two selection paths -- the logit-histogram fast path and the exact radix select it falls back to when more
than 1024 candidates remain -- and the contract (score descending, then flat index ascending; across classes: class, then per-class
rank) has to hold whichever of them runs. The regression maps label every box with its pixel (box[2] is the flat index), so a wrong
choice among tied pixels shows as a wrong index, not as an equal score.
"""
import ctypes

import numpy as np
import pytest
import torch

import ref_decode_edges as R
from cpd_amd import ops
from cpd_amd._lib import CpdHipError, farr, lib, ptr, stream

pytestmark = pytest.mark.gpu

CASES = R.cases()
SCORE_ATOL = 1e-6                       # device against host sigmoid: the bound tests/test_gpu_decode_nms.py uses for this kernel
DIM_ATOL = 1e-5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_decode(logits, k, limit_range=R.WIDE, score_thresh=-1.0):
    nc, h, w = logits.shape
    hm, center, cz, dim, rot = (dev(m) for m in (logits, *R.maps(h, w)))
    boxes, scores, labels, n = ops.center_decode(hm, center, cz, dim, rot, 1, h * w, nc, h, w, k, R.STRIDE, R.VOXEL, R.RANGE_LO,
                                                 limit_range, score_thresh)
    assert boxes.shape[0] == scores.shape[0] == labels.shape[0] == n
    return boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()


def oracle_decode(oracle, logits, k, limit_range=R.WIDE, score_thresh=-1.0):
    nc, h, w = logits.shape
    return oracle.center_decode(logits, *R.maps(h, w), k, R.STRIDE, R.VOXEL, R.RANGE_LO, limit_range, score_thresh)


def assert_same(got, want, score_atol=SCORE_ATOL):
    (gb, gs, gl), (wb, ws, wl) = got, want
    assert gb.shape[0] == wb.shape[0]                                          # the count
    np.testing.assert_array_equal(gb[:, 2].astype(np.int64), wb[:, 2].astype(np.int64))    # the pixel
    np.testing.assert_array_equal(gl, wl)
    np.testing.assert_array_equal(gb[:, [0, 1, 2, 6]], wb[:, [0, 1, 2, 6]])    # x, y, z, yaw: exact by construction
    np.testing.assert_allclose(gb[:, 3:6], wb[:, 3:6], atol=DIM_ATOL, rtol=0)
    np.testing.assert_allclose(gs, ws, atol=score_atol, rtol=0)
    assert (np.diff(gs) <= 0).all()


@pytest.fixture(scope="module")
def want(oracle):
    """The oracle's answer for every case, computed once."""
    return {name: oracle_decode(oracle, logits, k) for name, (logits, k, _) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_the_oracle(hip, want, name):
    logits, k, notes = CASES[name]
    if not notes["supported"]:                                # the issue's K = 37 + 2000 is beyond the kernel: refused, not decoded
        with pytest.raises(CpdHipError, match="CPD_ERR_UNSUPPORTED"):
            gpu_decode(logits, k)
        return
    got = gpu_decode(logits, k)
    assert got[0].shape[0] == k
    assert_same(got, want[name])


def test_near_saturation_ties_follow_the_devices_own_scores(hip):
    """Logits in (13, 16.5): fp32 sigmoid values a few ulp below 1.0f, where the host's and the device's expf may round apart and the
    host cannot say which pixels tie. K = H*W returns every pixel with the device's own score (checked against the host to 1e-6);
    K = 100 must then be the contract's order over exactly those values."""
    rng = np.random.default_rng(201)
    logits = R.saturated_map(rng, 32, 32, lo=13.0, hi=16.5, n_hot=300, infinities=False)
    boxes, scores, labels = gpu_decode(logits, 1024)
    pixel = boxes[:, 2].astype(np.int64)
    np.testing.assert_array_equal(np.sort(pixel), np.arange(1024))
    dev_sig = np.empty(1024, np.float32)
    dev_sig[pixel] = scores
    np.testing.assert_allclose(dev_sig, R.sigmoid32(logits).ravel(), atol=SCORE_ATOL, rtol=0)
    assert (np.diff(scores) <= 0).all() and (labels == 0).all()
    assert np.unique(dev_sig[logits.ravel() >= 13]).size < 150                # the point of the fixture: many ties among the 300
    np.testing.assert_array_equal(pixel, R.decode_ref(logits, 1024, sig=dev_sig)[3])
    b100, s100, l100 = gpu_decode(logits, 100)
    _, rs, _, rp = R.decode_ref(logits, 100, sig=dev_sig)
    np.testing.assert_array_equal(b100[:, 2].astype(np.int64), rp)
    np.testing.assert_array_equal(s100, rs)                                   # the same kernel arithmetic: bit for bit
    np.testing.assert_array_equal(b100, R.boxes_of(rp, 32))


def test_samples_of_one_launch_take_different_paths(oracle, hip):
    """batch = 3 in the engine's channels-last rows (16 floats per pixel, heat map in columns 8..10): an ordinary map, a constant map
    (radix path) and a saturated one, each against its own single-sample oracle result."""
    nc, h, w, k, ld = 3, 40, 30, 500, 16
    rng = np.random.default_rng(202)
    hot = np.concatenate([R.saturated_map(rng, h, w, n_hot=700, infinities=False) for _ in range(nc)])
    samples = [R.background(rng, (nc, h, w), 1.5, -1.0), np.zeros((nc, h, w), np.float32), hot]
    notes = [dict(fallback=False, saturated=False), dict(fallback=True, saturated=False), dict(fallback=False, saturated=True)]
    center, cz, dim, rot = R.maps(h, w)
    rows = np.zeros((3, h * w, ld), np.float32)
    for b, logits in enumerate(samples):
        R.check_conditions(logits, k, notes[b])
        planes = np.concatenate([center, cz, dim, rot, logits]).reshape(8 + nc, h * w)
        rows[b, :, :8 + nc] = planes.T
    t = dev(rows.reshape(3 * h * w, ld))
    boxes, scores, labels, counts = ops.center_decode(t[:, 8:], t[:, 0:], t[:, 2:], t[:, 3:], t[:, 6:], ld, 1, nc, h, w, k, R.STRIDE,
                                                      R.VOXEL, R.RANGE_LO, R.WIDE, 0.05, sync=False, batch=3, sample_stride=h * w * ld)
    counts = counts.cpu().numpy()
    boxes, scores, labels = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()
    for b, logits in enumerate(samples):
        n = int(counts[b])
        assert_same((boxes[b, :n], scores[b, :n], labels[b, :n]), oracle_decode(oracle, logits, k, R.WIDE, 0.05))
    assert counts[1] == k and counts[2] == k and 100 < counts[0] <= k


@pytest.fixture(scope="module")
def mask_map():
    """`quantised` moved down by its 50th largest logit: the 100 best then straddle logit 0, whose score is exactly 0.5 on the host
    and on the device (expf(0) == 1)."""
    q = CASES["quantised-k100"][0]
    shifted = q - np.sort(q.ravel())[::-1][49]
    R.check_conditions(shifted, 100, dict(fallback=False, saturated=False))
    return shifted


def test_limit_range_is_inclusive(oracle, hip, want):
    logits, k, _ = CASES["quantised-k100"]
    full = want["quantised-k100"]
    pick = full[0][50]                                        # a box from the middle of the list
    removed = 0
    for axis in range(3):
        for side in (0, 1):                                   # the lower bound, then the upper bound, on this box's coordinate
            for inward in (False, True):
                v = np.float32(pick[axis])
                if inward:
                    v = np.nextafter(v, np.float32(np.inf if side == 0 else -np.inf))
                lim = list(R.WIDE)
                lim[axis + 3 * side] = float(v)
                got = gpu_decode(logits, k, lim)
                assert_same(got, oracle_decode(oracle, logits, k, lim))
                assert (pick[2] in got[0][:, 2]) == (not inward)
                cut = (full[0][:, axis] < v) if side == 0 else (full[0][:, axis] > v)
                np.testing.assert_array_equal(got[0][:, 2], full[0][~cut, 2])      # compaction keeps the order
                np.testing.assert_array_equal(got[2], full[2][~cut])
                removed += int(cut.sum())
    assert removed > 100


def test_score_threshold_is_strict(oracle, hip, mask_map):
    k = 100
    full = oracle_decode(oracle, mask_map, k)
    half = np.float32(0.5)
    assert (full[1] > half).any() and (full[1] == half).any() and (full[1] < half).any()
    got = gpu_decode(mask_map, k, R.WIDE, 0.5)
    assert_same(got, oracle_decode(oracle, mask_map, k, R.WIDE, 0.5))
    assert got[0].shape[0] == (full[1] > half).sum() and (got[1] > half).all()     # the 0.5 pixels are dropped
    np.testing.assert_array_equal(got[0][:, 2], full[0][full[1] > half, 2])
    # the same threshold together with a limit that cuts boxes out of the middle
    lim = list(R.WIDE)
    lim[0] = float(np.median(full[0][:, 0]))
    got = gpu_decode(mask_map, k, lim, 0.5)
    assert_same(got, oracle_decode(oracle, mask_map, k, lim, 0.5))
    keep = (full[1] > half) & (full[0][:, 0] >= np.float32(lim[0]))
    assert 0 < keep.sum() < (full[1] > half).sum()
    np.testing.assert_array_equal(got[0][:, 2], full[0][keep, 2])


def test_threshold_extremes(oracle, hip, want):
    logits, k, _ = CASES["quantised-k100"]
    b, s, l = gpu_decode(logits, k, R.WIDE, 2.0)              # nothing passes: n == 0, no error
    assert b.shape == (0, 7) and s.shape == (0,) and l.shape == (0,)
    got = gpu_decode(logits, k, R.WIDE, -1.0)                 # everything passes: n == K
    assert got[0].shape[0] == k
    assert_same(got, want["quantised-k100"])
    b, _, _ = gpu_decode(logits, k, (5.0, 5.0, 5.0, -5.0, -5.0, -5.0))         # an empty limit range
    assert b.shape == (0, 7)


def raw_decode(logits, k, workspace_short=0):
    """cpd_center_decode called directly on buffers this test owns: (return code, outputs untouched?)."""
    nc, h, w = logits.shape
    hm, center, cz, dim, rot = (dev(m) for m in (logits, *R.maps(h, w)))
    need = lib().cpd_center_decode_workspace_bytes(1, nc, h * w, k)
    boxes = torch.full((k, 7), 7.5, device="cuda")
    scores = torch.full((k,), 7.5, device="cuda")
    labels = torch.full((k,), 77, dtype=torch.int32, device="cuda")
    n_out = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    ws = torch.full((max(need, 1),), 77, dtype=torch.uint8, device="cuda")
    rc = lib().cpd_center_decode(ptr(hm), ptr(center), ptr(cz), ptr(dim), ptr(rot), 1, 0, 1, h * w, nc, h, w, k, R.STRIDE,
                                 farr(R.VOXEL), farr(R.RANGE_LO), farr(R.WIDE), -1.0, ptr(boxes), ptr(scores), ptr(labels),
                                 ptr(n_out), ptr(ws), ctypes.c_size_t(need - workspace_short), stream())
    torch.cuda.synchronize()
    untouched = bool((boxes == 7.5).all() and (scores == 7.5).all() and (labels == 77).all() and (n_out == 77).all() and
                     (ws == 77).all())
    return rc, untouched


def test_error_returns_launch_nothing(hip):
    logits = CASES["whole_map_32x32-k1024"][0]
    tall = np.zeros((1, 40, 30), np.float32)
    small = CASES["whole_map_4x5-k20"][0]
    with pytest.raises(CpdHipError, match="CPD_ERR_UNSUPPORTED"):
        gpu_decode(tall, 1025)                                # k > 1024
    with pytest.raises(CpdHipError, match="CPD_ERR_UNSUPPORTED"):
        gpu_decode(small, 4 * 5 + 1)                          # k > h * w
    unsupported, workspace = -4, -2                           # CPD_ERR_UNSUPPORTED, CPD_ERR_WORKSPACE (include/cpd_hip.h)
    assert raw_decode(tall, 1025) == (unsupported, True)
    assert raw_decode(small, 21) == (unsupported, True)
    assert raw_decode(logits, 1024, workspace_short=1) == (workspace, True)
    rc, untouched = raw_decode(logits, 1024)                  # and the same call with the workspace it asked for runs
    assert rc == 0 and not untouched
