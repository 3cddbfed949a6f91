#!/usr/bin/env python3
"""Seed search for tests/ref_decode_peaks.py: a float64 restatement of the unmasked decode on the host, and for every shape and seed the
smallest distance of a decoded centre to the limit range and of a score to the threshold. A seed is fit when the first exceeds 1e-3
and the second 1e-6 by a wide margin (the GPU test asserts both on the device's own output):  python tools/decode_peaks_seeds.py [n_seeds]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import ref_decode_peaks as R                                   # noqa: E402
from ref_decode_peaks import C_HID, N_REG, NUM_CLASS, STRIDE, VOXEL, geometry          # noqa: E402


def reg_maps_f64(d):
    """the four regression maps as the last convolution over the zero-padded hidden map, in float64 -> [B, h, w, 8]"""
    B, h, w = d["B"], d["h"], d["w"]
    pad = np.zeros((B, h + 2, w + 2, C_HID))
    pad[:, 1:-1, 1:-1] = d["hidden"]
    out = np.tile(d["bias"].astype(np.float64), (B, h, w, 1))
    for t in range(9):
        out += pad[:, t // 3:t // 3 + h, t % 3:t % 3 + w] @ d["w_last"][t].astype(np.float64)
    return out


def host_decode(d):
    """float64 restatement of the unmasked decode (random maps: no ties) -> (centres [B, K, 3], scores [B, K])"""
    B, h, w, K = d["B"], d["h"], d["w"], d["K"]
    lo, _ = geometry(h, w)
    reg = reg_maps_f64(d).reshape(B, h * w, N_REG)
    s = 1.0 / (1.0 + np.exp(-d["hm"].astype(np.float64))).reshape(B, h * w, NUM_CLASS)
    centres, scores = np.zeros((B, K, 3)), np.zeros((B, K))
    for b in range(B):
        cand = []
        for c in range(NUM_CLASS):
            top = np.argsort(-s[b, :, c], kind="stable")[:K]
            cand += [(s[b, i, c], i) for i in top]
        cand.sort(key=lambda v: -v[0])
        for k, (sc, i) in enumerate(cand[:K]):
            centres[b, k] = [(i % w + reg[b, i, 0]) * STRIDE * VOXEL[0] + lo[0], (i // w + reg[b, i, 1]) * STRIDE * VOXEL[1] + lo[1], reg[b, i, 2]]
            scores[b, k] = sc
    return centres, scores



if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    for name, (B, h, w, K, chosen) in list(R.SHAPES.items()):
        for seed in range(1, n + 1):
            R.SHAPES[name] = (B, h, w, K, seed)
            d = R.draw(name)
            centres, scores = host_decode(d)
            lim = np.asarray(geometry(h, w)[1])
            c = centres.reshape(-1, 3)
            kept = ((c >= lim[:3]) & (c <= lim[3:])).all(1) & (scores.reshape(-1) > R.SCORE_THRESH)
            m = R.margins(centres, scores, lim)
            print("%-16s seed %d%s  centre margin %.4f  score margin %.5f  kept %d of %d" % (name, seed, " *" if seed == chosen else "  ", m[0], m[1],
                                                                                         kept.sum(), kept.size))
        R.SHAPES[name] = (B, h, w, K, chosen)
