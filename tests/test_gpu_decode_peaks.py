"""The CenterHead decode cut at the peaks (cpd_center_peaks -> cpd_peak_rulebook -> cpd_center_decode_at_peaks) against
cpd_center_decode on the full maps. Synthetic maps (tests/ref_decode_peaks.py), no convolution kernel involved: the regression maps of
the full decode are torch's conv2d of the hidden map (padding 1, float64 then float32); the peaks path gets the hidden rows gathered
in torch through the table's centre column, rows of a site outside the image filled with 1e3 -- the last convolution pads the hidden
map with ZEROS, so a finish that does not skip those taps is off by hundreds.

Counts, labels, scores and peak pixels must be identical; boxes within 1e-5 absolute (the last convolution's fp32 summation order
against float64 rounded once; regression values of ~0.5, box coordinates below 20).
"""
import numpy as np
import pytest
import torch

import ref_decode_peaks as R
from cpd_amd import ops
from cpd_amd._lib import farr, iarr, lib, ptr, stream

pytestmark = pytest.mark.gpu

BOX_ATOL = 1e-5
WIDE = [-1e6] * 3 + [1e6] * 3


class Case:
    """one shape's device tensors and the outputs both paths share"""

    def __init__(self, name):
        d = self.d = R.draw(name)
        B, h, w, K = self.shape = (d["B"], d["h"], d["w"], d["K"])
        self.lo, self.lim = R.geometry(h, w)
        hid = torch.from_numpy(d["hidden"]).cuda()
        w_last = torch.from_numpy(d["w_last"]).cuda()
        bias = torch.from_numpy(d["bias"]).cuda()
        wt = w_last.view(3, 3, R.C_HID, R.N_REG).permute(3, 2, 0, 1).double()
        reg = torch.nn.functional.conv2d(hid.permute(0, 3, 1, 2).double(), wt, bias.double(), padding=1).float()      # [B, 8, h, w]
        rows = torch.zeros((B * h * w, R.LD), dtype=torch.float32, device="cuda")
        rows[:, :R.N_REG] = reg.permute(0, 2, 3, 1).reshape(B * h * w, R.N_REG)
        rows[:, 8:8 + R.NUM_CLASS] = torch.from_numpy(d["hm"]).cuda().view(B * h * w, R.NUM_CLASS)
        self.rows, self.hid_rows, self.w_last, self.bias = rows, hid.view(B * h * w, R.C_HID), w_last.contiguous(), bias
        # the full maps' pixel labels: a second set of rows whose center_z is the flat pixel index (exact in fp32)
        lab = rows.clone()
        lab[:, :R.N_REG] = 0
        lab[:, 2] = torch.arange(h * w, device="cuda", dtype=torch.float32).repeat(B)
        self.lab_rows = lab

    def full(self, rows, lim, thresh):
        B, h, w, K = self.shape
        o = R.OFFSETS
        out = ops.center_decode(rows[:, 8:], rows[:, o[0]:], rows[:, o[1]:], rows[:, o[2]:], rows[:, o[3]:], R.LD, 1, R.NUM_CLASS, h, w, K,
                                R.STRIDE, R.VOXEL, self.lo, lim, thresh, sync=False, batch=B, sample_stride=h * w * R.LD)
        return [t.cpu().numpy() for t in out]

    def peaks(self):
        B, h, w, K = self.shape
        return ops.center_peaks(self.rows[:, 8:], R.LD, 1, R.NUM_CLASS, h, w, K, batch=B, sample_stride=h * w * R.LD)

    def at_peaks(self, lim, thresh, garbage=1e3):
        B, h, w, K = self.shape
        score, cand, ind = self.peaks()
        nbr = ops.peak_rulebook(ind, h, w)
        site = nbr[4].long()                                   # the centre tap: the hidden site's own row, -1 outside the image
        hidden = torch.full((B * K * 9, R.C_HID), garbage, dtype=torch.float32, device="cuda")
        hidden[site >= 0] = self.hid_rows[site[site >= 0]]
        out = ops.center_decode_at_peaks(score, cand, ind, hidden, R.C_HID, self.w_last, self.bias, R.OFFSETS, R.NUM_CLASS, h, w, R.STRIDE,
                                         R.VOXEL, self.lo, lim, thresh)
        return [t.cpu().numpy() for t in out], (score.cpu().numpy(), cand.cpu().numpy(), ind.cpu().numpy(), nbr.cpu().numpy())


@pytest.fixture(scope="module")
def cases(hip):
    return {name: Case(name) for name in R.SHAPES}


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_selection_is_the_full_decodes(cases, name):
    c = cases[name]
    B, h, w, K = c.shape
    boxes, scores, labels, n = c.full(c.lab_rows, WIDE, -1.0)
    assert (n == K).all()
    score, cand, ind = (t.cpu().numpy() for t in c.peaks())
    np.testing.assert_array_equal(score, scores)
    np.testing.assert_array_equal(cand // K, labels)
    np.testing.assert_array_equal(ind, boxes[:, :, 2].astype(np.int64))
    assert ((ind >= 0) & (ind < h * w)).all()
    if name == "all_pixels_5x7":
        # K = h * w candidates per class, merged over three classes: most pixels of a frame are peaks -- the four corners and inner
        # pixels of every edge among them
        assert all(len(set(ind[b])) > 20 for b in range(B))
        seen = set(int(i) for i in ind.reshape(-1))
        assert {0, w - 1, (h - 1) * w, h * w - 1} <= seen
        for edge in (range(1, w - 1), range((h - 1) * w + 1, h * w - 1), range(w, (h - 1) * w, w), range(2 * w - 1, h * w - 1, w)):
            assert seen & set(edge)


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_table_matches_numpy(cases, name):
    c = cases[name]
    B, h, w, K = c.shape
    _, (_, _, ind, nbr) = c.at_peaks(WIDE, -1.0)
    want = R.rulebook(ind, h, w)
    np.testing.assert_array_equal(nbr, want)
    frame = np.repeat(np.arange(B), K * 9)[None, :]
    inside = nbr >= 0
    assert (((nbr // (h * w)) == frame) | ~inside).all()                      # no neighbour in another frame
    outside_site = nbr[4] < 0
    assert outside_site.any() and (nbr[:, outside_site] == -1).all()           # a hidden site outside the image: all nine columns


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_boxes_match_the_full_decode(cases, name):
    c = cases[name]
    B, h, w, K = c.shape
    # the reference's own unmasked output: no centre near a limit, no score near the threshold -> no mask can flip inside BOX_ATOL
    rb, rs, _, rn = c.full(c.rows, WIDE, -1.0)
    assert (rn == K).all()
    m_lim, m_score = R.margins(rb[:, :, :3], rs, c.lim)
    print("%s: centre margin %.3g, score margin %.3g" % (name, m_lim, m_score))
    assert m_lim > 1e-3 and m_score > 1e-6
    for lim, thresh in ((WIDE, -1.0), (c.lim, R.SCORE_THRESH)):
        wb, ws, wl, wn = c.full(c.rows, lim, thresh)
        (gb, gs, gl, gn), _ = c.at_peaks(lim, thresh)
        np.testing.assert_array_equal(gn, wn)
        if lim is not WIDE:
            assert (wn < K).any() and (wn > 0).all()               # the masks do cut
        for b in range(B):
            n = int(wn[b])
            np.testing.assert_array_equal(gl[b, :n], wl[b, :n])
            np.testing.assert_array_equal(gs[b, :n], ws[b, :n])
            err = np.abs(gb[b, :n] - wb[b, :n])
            err[:, 6] = np.minimum(err[:, 6], 2 * np.pi - err[:, 6])
            print("%s frame %d: %d boxes, max |box error| %.3g" % (name, b, n, err.max() if n else 0.0))
            assert err.max() <= BOX_ATOL


def test_zero_rows_give_the_same_boxes(cases):
    """the skipped taps really are skipped: zeros instead of 1e3 in the outside rows change no bit"""
    c = cases["all_pixels_5x7"]
    (a, _, _, _), _ = c.at_peaks(WIDE, -1.0, garbage=1e3)
    (b, _, _, _), _ = c.at_peaks(WIDE, -1.0, garbage=0.0)
    np.testing.assert_array_equal(a, b)


def test_argument_errors_match_center_decode(hip):
    nc, h, w = 3, 4, 4
    dev = "cuda"
    hm = torch.zeros((h * w, 16), device=dev)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    vox, lo, lim = farr(R.VOXEL), farr([0, 0]), farr(WIDE)

    def full(k, hm_t=hm):
        return lib().cpd_center_decode(ptr(hm_t), ptr(hm), ptr(hm), ptr(hm), ptr(hm), 1, 0, 16, 1, nc, h, w, k, R.STRIDE, vox, lo, lim, 0.1,
                                       ptr(f(k, 7)), ptr(f(k)), ptr(i(k)), ptr(i(1)), ptr(ws), ws.numel(), stream())

    def peaks(k, hm_t=hm, ws_bytes=None):
        return lib().cpd_center_peaks(ptr(hm_t), 1, 0, 16, 1, nc, h, w, k, ptr(f(k)), ptr(i(k)), ptr(i(k)), ptr(ws),
                                      ws.numel() if ws_bytes is None else ws_bytes, stream())

    def finish(k, hidden, ws_bytes=None):
        return lib().cpd_center_decode_at_peaks(ptr(f(k)), ptr(i(k)), ptr(i(k)), ptr(hidden), R.C_HID, R.C_HID, ptr(f(9, R.C_HID, 8)), ptr(f(8)), 8,
                                                iarr(R.OFFSETS), 1, nc, h, w, k, R.STRIDE, vox, lo, lim, 0.1, ptr(f(k, 7)), ptr(f(k)), ptr(i(k)),
                                                ptr(i(1)), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, stream())

    assert full(h * w + 1) == peaks(h * w + 1) == finish(h * w + 1, f((h * w + 1) * 9, R.C_HID)) == -4       # k > h * w
    assert lib().cpd_peak_rulebook(ptr(i(h * w + 1)), 1, h * w + 1, h, w, ptr(i(9, (h * w + 1) * 9)), stream()) == -4
    assert full(4, None) == peaks(4, None) == finish(4, None) == -1                                            # null pointers
    assert lib().cpd_peak_rulebook(None, 1, 4, h, w, ptr(i(9, 36)), stream()) == -1
    assert peaks(4, ws_bytes=8) == finish(4, f(36, R.C_HID), ws_bytes=8) == -2                                 # workspace too small
    assert full(4) == peaks(4) == finish(4, f(36, R.C_HID)) == 0
    torch.cuda.synchronize()
