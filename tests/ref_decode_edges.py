"""Fixtures and a plain numpy restatement for the CenterHead decode (cpd_center_decode) on tied, saturated and degenerate heat maps.

The decode's contract (cpd_amd/csrc/decode.hip, oracle/cpd_oracle.c): fp32 sigmoid of the logits; per class the K best pixels in
(score descending, flat index ascending) order; across classes the K best of those in (score descending, class ascending, per-class
rank ascending) order; the inclusive POST_CENTER_LIMIT_RANGE mask and the strict `score > thresh` mask; order-preserving compaction.

`cases()` builds heat maps from seeds at the smallest shapes at which each selection path of topk_class_kernel can still go wrong, and
`maps()` builds regression maps that make every picked pixel identifiable without touching the arithmetic under test:
center_z[ind] = ind (exact below 2^24) so box[2] IS the flat index; center = 0, dim = 0, rot = (cos 1, sin 0); stride 8 x voxel 0.125
with range_lo -64 so x = ind % w - 64 and y = ind // w - 64 are exact in fp32 with or without FMA contraction.

Every fixture is built so that the reference alone decides the answer on any host and on the device (check_conditions):
  * two DISTINCT fp32 sigmoid values of one fixture are >= 16 ulp apart, so the 1-2 ulp between two expf implementations can reorder
    nothing; what remains equal is equal by construction (equal logits) or saturated (logit >= 18: 1 + expf(-x) rounds to 1.0f, +inf
    -> 1.0f and -inf -> 0.0f on both sides);
  * the cases marked `fallback` place more than 1024 pixels at or within one histogram-bin width of the K-th logit, more than the fast
    path's candidate buffer holds, so the exact radix select (block_topk) is what runs.

NaN logits are left out on purpose: the order of NaN scores is unspecified in the reference (torch.topk), the oracle's qsort
comparator is not a total order on NaN, and the device's key transform puts NaN wherever its sign bit says. A NaN heat map is a broken
network, not a decode case; nothing here promises an order for it.
"""
import ctypes
import ctypes.util

import numpy as np

KMAX = 1024                              # cpd_center_decode refuses k > 1024
BIN_WIDTH = 40.0 / 2048                  # topk_class_kernel's logit histogram: 2048 linear bins over [-20, 20)
STRIDE, VOXEL, RANGE_LO = 8.0, (0.125, 0.125), (-64.0, -64.0)
WIDE = (-1e9, -1e9, -1e9, 1e9, 1e9, 1e9)  # a limit range that masks nothing
MIN_ULP_GAP = 16

_expf = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").expf
_expf.restype, _expf.argtypes = ctypes.c_float, [ctypes.c_float]


def sigmoid32(x):
    """1.0f / (1.0f + expf(-x)) in fp32, with the C library's expf (the function the oracle calls: numpy's own float32 exp is a
    different implementation and may differ from it in the last bit)."""
    x = np.asarray(x, np.float32)
    u, inv = np.unique(x.ravel(), return_inverse=True)
    e = np.array([_expf(float(-v)) for v in u], np.float32)
    with np.errstate(over="ignore"):
        s = (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)
    return s[inv].reshape(x.shape)


def topk_order(score, k):
    """(score descending, index ascending), first k -- on the rows of a 2-D array or on a 1-D array."""
    score = np.asarray(score)
    if score.ndim == 1:
        return np.lexsort((np.arange(score.size), -score.astype(np.float64)))[:k]
    return np.stack([topk_order(r, k) for r in score])


def two_stage_topk(sig, k):
    """sig [nc, hw] fp32 scores -> (scores[k], labels[k], pixel[k]) of the two-stage top-K."""
    nc, hw = sig.shape
    i1 = topk_order(sig, k)                                   # [nc, k] pixel per (class, rank)
    s1 = np.take_along_axis(sig, i1, 1)
    cls, rank = np.divmod(np.arange(nc * k), k)
    o = np.lexsort((rank, cls, -s1.ravel().astype(np.float64)))[:k]
    return s1.ravel()[o], cls[o].astype(np.int32), i1.ravel()[o].astype(np.int64)


def maps(h, w):
    """The regression maps that label a box with its pixel: (center[2,h,w], center_z[1,h,w], dim[3,h,w], rot[2,h,w])."""
    assert h * w < (1 << 24)
    center = np.zeros((2, h, w), np.float32)
    center_z = np.arange(h * w, dtype=np.float32).reshape(1, h, w)
    dim = np.zeros((3, h, w), np.float32)
    rot = np.stack([np.ones((h, w), np.float32), np.zeros((h, w), np.float32)])
    return center, center_z, dim, rot


def boxes_of(pixel, w):
    """What the decode makes of maps() at the given pixels: exact in fp32."""
    pixel = np.asarray(pixel, np.int64)
    b = np.zeros((pixel.size, 7), np.float32)
    b[:, 0] = (pixel % w).astype(np.float32) - 64.0
    b[:, 1] = (pixel // w).astype(np.float32) - 64.0
    b[:, 2] = pixel.astype(np.float32)
    b[:, 3:6] = 1.0
    return b


def decode_ref(logits, k, limit_range=WIDE, score_thresh=-1.0, sig=None):
    """The numpy restatement of the whole decode on maps(): (boxes[n,7], scores[n], labels[n], pixel[n]). `sig` replaces the host's
    fp32 sigmoid of the logits (the near-saturation test passes the device's own values)."""
    nc, h, w = logits.shape
    sig = sigmoid32(logits).reshape(nc, h * w) if sig is None else np.asarray(sig, np.float32).reshape(nc, h * w)
    scores, labels, pixel = two_stage_topk(sig, k)
    boxes = boxes_of(pixel, w)
    lim = np.asarray(limit_range, np.float32)
    keep = (boxes[:, :3] >= lim[:3]).all(1) & (boxes[:, :3] <= lim[3:]).all(1) & (scores > np.float32(score_thresh))
    return boxes[keep], scores[keep], labels[keep], pixel[keep]


def logit_bin(x):
    """topk_class_kernel's histogram bin of a logit (decode.hip, logit_bin)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, np.float32) + np.float32(20.0)) * np.float32(51.2)
    return np.clip(t, 0.0, 2047.0).astype(np.int64)


def bin_then_sort_topk(logits_c, k):
    """The rule the contract does NOT allow, restated: take the pixels of one class whose logit bin is >= the bin b* that holds the
    K-th logit, and only then order them by (sigmoid key descending, index ascending). Returns the chosen pixels, or None where more
    than 1024 pixels lie in bins >= b* (the kernel then runs its exact path). Kept to show that `saturated` separates the two rules."""
    x = np.asarray(logits_c, np.float32).ravel()
    b = logit_bin(x)
    bstar = np.sort(b)[::-1][k - 1]
    cand = np.nonzero(b >= bstar)[0]
    if cand.size > 1024:
        return None
    return cand[topk_order(sigmoid32(x[cand]), k)]


# ---------------------------------------------------------------------------------------------------------------- fixtures
def background(rng, shape, scale=1.0, shift=0.0):
    """A normally distributed map on a 1/256 grid, clipped to [-12, 8]: up to logit 8 one grid step moves the sigmoid by more than
    16 ulp (1/256 * sigmoid'(8) = 1.3e-6 against 16 * 2^-24 = 9.5e-7), and below 0 the steps only get wider relative to an ulp."""
    x = np.clip(rng.normal(size=shape) * scale + shift, -12.0, 8.0)
    return (np.round(x * 256.0) / 256.0).astype(np.float32)


def quantised(rng, shape, sigma=2.5):
    """Multiples of 1/8 in [-8, 8], bell-shaped so that the best K span several levels: many exact ties inside and across classes,
    a handful of pixels per class at the clipped top level."""
    return (np.clip(np.round(rng.normal(size=shape) * sigma * 8.0), -64, 64) / 8.0).astype(np.float32)


def saturated_map(rng, h, w, lo=18.0, hi=19.9, n_hot=150, infinities=True, scale=1.0):
    x = background(rng, (1, h, w), scale).reshape(-1)
    pick = rng.permutation(h * w)
    hot, cold = pick[:n_hot], pick[n_hot:]
    x[hot] = rng.uniform(lo, hi, n_hot).astype(np.float32)
    if infinities:
        x[hot[:3]] = np.inf
        x[cold[:3]] = -np.inf
    return x.reshape(1, h, w)


def tie_group_map(rng, h, w, n_high, n_tied, level, n_near=0):
    """`n_high` distinct levels above `level`, `n_tied` copies of `level`, `n_near` distinct levels within a third of a bin width
    below it, the rest clearly lower; shuffled."""
    n = h * w
    high = level + 0.5 + np.arange(n_high) / 16.0
    near = level - (1 + np.arange(n_near)) * 2.0 ** -15
    assert n_near * 2.0 ** -15 < BIN_WIDTH / 3
    low = background(rng, n - n_high - n_tied - n_near, 1.0, level - 6.0)
    x = np.concatenate([high, np.full(n_tied, level), near, low]).astype(np.float32)
    return rng.permutation(x).reshape(1, h, w)


def cases():
    """name -> (logits [nc,h,w] fp32, K, notes). notes: `fallback` -- the fixture forces the exact radix path (more than 1024 pixels at
    or within one bin width of the K-th logit of every class); `saturated` -- the winners all score exactly 1.0f; `supported` -- False
    where cpd_center_decode refuses the K (k > 1024) and only the oracle and the restatement can be compared."""
    out = {}

    def add(name, logits, k, **notes):
        notes = dict(dict(fallback=False, saturated=False, supported=k <= KMAX), **notes)
        out["%s-k%d" % (name, k)] = (np.ascontiguousarray(logits, np.float32), k, notes)

    for k in (1, 7, 500, 1024):                               # 1200 px: no multiple of 1024 or of 64
        add("const", np.zeros((3, 40, 30), np.float32), k, fallback=True)
    add("const_per_class", np.broadcast_to(np.arange(-1.0, 2.0, dtype=np.float32)[:, None, None], (3, 40, 30)), 500, fallback=True)
    tg = tie_group_map(np.random.default_rng(101), 64, 64, 37, 2000, 0.3)
    for k in (100, 38, 37 + 2000):                            # remaining = 63, 1, and the whole group (beyond the kernel's K)
        add("tie_group", tg, k, fallback=True)
    # the whole tie group taken at a K the kernel accepts: 37 above + 987 tied = 1024, 200 more just below keep the radix path
    add("tie_group_whole", tie_group_map(np.random.default_rng(102), 64, 64, 37, 987, 1.01, n_near=200), 1024, fallback=True)
    ob = np.random.default_rng(103).permutation(np.linspace(0.001, 0.018, 2048).astype(np.float32)).reshape(1, 32, 64)
    for k in (100, 1024):
        add("one_bin", ob, k, fallback=True)
    add("saturated", saturated_map(np.random.default_rng(104), 64, 64), 100, saturated=True)
    q = quantised(np.random.default_rng(105), (3, 64, 64))
    for k in (1, 100, 500):
        add("quantised", q, k)
    add("whole_map_4x5", quantised(np.random.default_rng(106), (3, 4, 5)), 20)
    add("whole_map_32x32", quantised(np.random.default_rng(107), (1, 32, 32)), 1024)
    add("identical_classes", np.repeat(quantised(np.random.default_rng(108), (1, 8, 8)), 5, axis=0), 64)
    return out


def min_ulp_gap(sig):
    """The smallest distance, in fp32 steps, between two distinct values of a non-negative fp32 array."""
    u = np.unique(np.asarray(sig, np.float32).ravel())
    assert (u >= 0).all()
    bits = u.view(np.int32).astype(np.int64)                  # monotone for non-negative floats
    return int(np.diff(bits).min()) if u.size > 1 else 1 << 31


def near_kth_count(logits_c, k):
    """Pixels of one class at or within one histogram-bin width of the K-th logit (or above it)."""
    x = np.asarray(logits_c, np.float32).ravel().astype(np.float64)
    kth = np.sort(x)[::-1][k - 1]
    return int((x >= kth - BIN_WIDTH).sum())


def check_conditions(logits, k, notes):
    """The conditions under which the reference alone decides the answer; raises AssertionError otherwise."""
    nc, h, w = logits.shape
    assert not np.isnan(logits).any() and 1 <= k <= h * w
    sig = sigmoid32(logits)
    assert min_ulp_gap(sig) >= MIN_ULP_GAP, min_ulp_gap(sig)
    hot = logits[sig == np.float32(1.0)]
    assert hot.size == 0 or hot.min() >= 18.0                 # 1.0f only where both sides saturate
    if notes["saturated"]:
        assert (two_stage_topk(sig.reshape(nc, -1), k)[0] == np.float32(1.0)).all()
        assert (sig == np.float32(1.0)).sum() > k             # and more of them than K: the index rule decides
    if notes["fallback"]:
        for c in range(nc):
            assert near_kth_count(logits[c], k) > 1024, (c, near_kth_count(logits[c], k))
