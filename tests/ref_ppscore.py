"""Numpy restatement of CPD's PP-score precompute (cpd/unsupervised_core/precompute_ppscore.py): the two rigid transforms with
their float32 roundings, the per-traversal fixed-radius neighbour counts, the normalised entropy and save_pp_score's window
loop. tests/golden/make_golden_ppscore.py asserts that it reproduces the reference (transformed coordinates and counts bit
for bit, float16 H on every point); the GPU tests use it on hand-built cases."""
import numpy as np


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """Correctly rounded a * b + c on float64 arrays without a hardware fma: exact product and sums as pairs, the low parts
    added with rounding to odd, then one rounding to nearest (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums")."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p, e = _two_prod(a, b)
    s, t = _two_sum(p, c)
    u, v = _two_sum(t, e)
    even = (np.ascontiguousarray(u).view(np.int64) & 1) == 0
    u = np.where((v != 0) & even, np.nextafter(u, np.where(v > 0, np.inf, -np.inf)), u)
    return s + u


def rigid(cloud, pose):
    """points_rigid_transform (l.36-45): [N, >=3] -> [N, 3] float32. The np.mat product of the float64 pose with the float32
    homogeneous cloud is a dgemm that accumulates over k with fused multiply-adds: m0 x, fma(m1, y, .), fma(m2, z, .), + m3;
    the result is rounded to float32."""
    cloud = np.asarray(cloud)
    if cloud.shape[0] == 0:
        return cloud
    p = cloud[:, 0:3].astype(np.float32).astype(np.float64)
    m = np.asarray(pose, np.float64)
    out = np.empty((p.shape[0], 3), np.float32)
    for r in range(3):
        out[:, r] = fma(m[r, 2], p[:, 2], fma(m[r, 1], p[:, 1], m[r, 0] * p[:, 0])) + m[r, 3]
    return out


def rigid_unfused(cloud, pose):
    """The same product with separately rounded multiplies and adds, (m0 x + m1 y) + m2 z + m3: NOT what the reference
    computes where the sum cancels (make_golden_ppscore.py prints how many coordinates differ)."""
    p = np.asarray(cloud)[:, 0:3].astype(np.float32).astype(np.float64)
    m = np.asarray(pose, np.float64)
    out = np.empty((p.shape[0], 3), np.float32)
    for r in range(3):
        out[:, r] = ((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3]
    return out


def _cells(xyz, r):
    return np.floor(xyz.astype(np.float64) / r).astype(np.int64)


def _key(c):
    o = 1 << 20
    return ((c[:, 0] + o) << 42) | ((c[:, 1] + o) << 21) | (c[:, 2] + o)


def count_one(query, pts, r):
    """Per query row the number of `pts` rows with float64 (dx dx + dy dy) + dz dz <= r r (cKDTree.query_ball_point(...,
    return_length=True): inclusive), through a sorted uniform grid of side r."""
    q = np.asarray(query)[:, 0:3].astype(np.float64)
    p = np.asarray(pts)[:, 0:3].astype(np.float64) if len(pts) else np.zeros((0, 3))
    out = np.zeros(len(q), np.int64)
    if len(q) == 0 or len(p) == 0:
        return out
    pk = _key(_cells(p, r))
    order = np.argsort(pk, kind="stable")
    pk, p = pk[order], p[order]
    qc = _cells(q, r)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = _key(qc + np.array([dx, dy, dz]))
                lo, hi = np.searchsorted(pk, k, "left"), np.searchsorted(pk, k, "right")
                n = hi - lo
                qi = np.repeat(np.arange(len(q)), n)
                if len(qi) == 0:
                    continue
                mi = np.arange(len(qi)) - np.repeat(np.cumsum(n) - n, n) + np.repeat(lo, n)
                d = q[qi] - p[mi]
                near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r * r
                out += np.bincount(qi[near], minlength=len(q))
    return out


def count_neighbors(query, traversals, r=0.3):
    """[N, T] int64 (count_neighbors, l.8-14)."""
    if len(traversals) == 0:
        return np.zeros((len(query), 0), np.int64)
    return np.stack([count_one(query, t, r) for t in traversals], 1)


def ephe_score(count):
    """compute_ephe_score (l.16-21) in float64. The reference's count array is the transpose of a stack, so its sum over
    axis 1 adds whole columns in traversal order: restated as that loop."""
    count = np.asarray(count)
    n = count.shape[1]
    P = count / (np.expand_dims(count.sum(axis=1), -1) + 1e-8)
    terms = -P * np.log(P + 1e-8)
    H = terms[:, 0].copy() if n else np.zeros(len(count))
    for t in range(1, n):
        H = H + terms[:, t]
    with np.errstate(divide="ignore", invalid="ignore"):
        return H / np.log(n)


def window(i, n_frames, max_win=30, win_inte=5):
    """The frames save_pp_score (l.77-94) loads for current frame i when files 0000 .. n_frames-1 exist."""
    return [j for j in range(i - max_win, i + max_win, win_inte) if 0 <= j < n_frames]


def frame_traversals(frames, poses, i, max_win=30, win_inte=5):
    """The traversals of current frame i in its own coordinates: sweep -> world -> frame i, float32 after each product."""
    inv = np.linalg.inv(poses[i])
    return [rigid(rigid(frames[j][:, 0:3], poses[j]), inv) for j in window(i, len(frames), max_win, win_inte)]


def sequence_ppscore(frames, poses, max_win=30, win_inte=5, r=0.3):
    """Per frame (counts [N, T] int64, H [N] float64)."""
    out = []
    for i in range(len(frames)):
        c = count_neighbors(frames[i][:, 0:3], frame_traversals(frames, poses, i, max_win, win_inte), r)
        out.append((c, ephe_score(c)))
    return out


def tie_mask(H, tol=1e-9):
    """Points whose float64 H lies within `tol` of a float16 rounding tie (the midpoint of two neighbouring float16 values)."""
    H = np.asarray(H, np.float64)
    h = H.astype(np.float16)
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    h = h.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.minimum(np.abs(H - (h + up) / 2), np.abs(H - (h + dn) / 2)) <= tol


def half_steps(a, b):
    """Distance of two float16 arrays in float16 steps (ordered-integer keys)."""
    def key(x):
        u = np.asarray(x, np.float16).view(np.uint16).astype(np.int64)
        return np.where(u & 0x8000, -(u & 0x7fff), u)
    return np.abs(key(a) - key(b))
