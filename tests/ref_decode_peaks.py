"""Fixtures and numpy restatements for the CenterHead decode cut at the peaks (cpd_center_peaks -> cpd_peak_rulebook ->
cpd_center_decode_at_peaks): synthetic heat maps, a hidden map and block-diagonal last-conv weights; no convolution kernel involved.

The seeds are chosen (tools/decode_peaks_seeds.py, a float64 restatement run on the host) so that no decoded centre lies within 1e-3 of the limit range and no score within
1e-6 of the threshold: a mask can then not flip inside the box tolerance. The GPU test asserts the same on the device's own output.
"""
import numpy as np

NUM_CLASS = 3
C_HID = 256
N_REG = 8
OFFSETS = [0, 2, 3, 6]                   # center (2), center_z (1), dim (3), rot (2) among the 8 regression values
WIDTHS = [2, 1, 3, 2]
STRIDE = 8.0
VOXEL = [0.1, 0.1]
SCORE_THRESH = 0.1
LD = 16                                  # row pitch of the full head rows: regression values in 0..7, hm in 8..10

#         name: (B, h, w, K, seed)
SHAPES = {"all_pixels_5x7": (3, 5, 7, 35, 4),          # every pixel a candidate: four corners, every edge, frame boundaries in the table
          "16x16": (2, 16, 16, 50, 5),
          "one_row_1x40": (1, 1, 40, 40, 5)}           # every vertical neighbour is outside


def geometry(h, w):
    """(range_lo_xy, limit_range): the map centred on the origin, limits that cut a strip off every side and both ends of z"""
    px = STRIDE * VOXEL[0]
    lo = [-0.5 * w * px, -0.5 * h * px]
    lim = [lo[0] + 0.9 * px, lo[1] + (0.6 * px if h > 1 else -1.0), -0.8, -lo[0] - 0.7 * px, -lo[1] - (0.8 * px if h > 1 else -1.0), 0.9]
    return lo, lim


def draw(name):
    B, h, w, K, seed = SHAPES[name]
    rng = np.random.default_rng(seed)
    hm = rng.normal(-3.5, 1.5, (B, h, w, NUM_CLASS)).astype(np.float32)
    hidden = np.maximum(rng.normal(0.0, 1.0, (B, h, w, C_HID)), 0.0).astype(np.float32)
    w_last = np.zeros((9, C_HID, N_REG), np.float32)
    cb = C_HID // 4
    for i, (o, n) in enumerate(zip(OFFSETS, WIDTHS)):
        w_last[:, i * cb:(i + 1) * cb, o:o + n] = rng.normal(0.0, 0.03, (9, cb, n))
    bias = rng.normal(0.0, 0.1, N_REG).astype(np.float32)
    return dict(B=B, h=h, w=w, K=K, hm=hm, hidden=hidden, w_last=w_last, bias=bias)


def rulebook(ind, h, w):
    """numpy construction of cpd_peak_rulebook's table from ind [B, K] -> [9, B * K * 9]"""
    B, K = ind.shape
    n = B * K * 9
    nbr = np.full((9, n), -1, np.int32)
    for b in range(B):
        for k in range(K):
            y, x = divmod(int(ind[b, k]), w)
            for t in range(9):
                sy, sx = y + t // 3 - 1, x + t % 3 - 1
                if not (0 <= sy < h and 0 <= sx < w):
                    continue
                for u in range(9):
                    iy, ix = sy + u // 3 - 1, sx + u % 3 - 1
                    if 0 <= iy < h and 0 <= ix < w:
                        nbr[u, (b * K + k) * 9 + t] = (b * h + iy) * w + ix
    return nbr


def margins(centres, scores, lim):
    """(smallest distance of a centre coordinate to its limits, smallest distance of a score to the threshold)"""
    lim = np.asarray(lim, np.float64)
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    return float(min(np.abs(c - lim[:3]).min(), np.abs(c - lim[3:]).min())), float(np.abs(np.asarray(scores, np.float64) - SCORE_THRESH).min())
