"""What tests/test_box_exact_ref.py (CPU restatements) and tests/test_gpu_box_exact.py (kernels) share around the exact
geometry of tests/ref_box_exact.py: the assertions every fp32 result goes through, the relabellings of a set, the KITTI
column mappings, and the seeded sets. Every set is chosen on the CPU from the exact geometry alone; the seed advances
until a set meets its condition, so no case is ever skipped.
"""
import numpy as np

from ref_box_exact import SHELL, Exact, general_position, worst_ratio


def assert_within(got, e, kind, label=""):
    """The check every fp32 box_geom result goes through: finite; clear pairs (no corner in the margin shell) within
    tol of the exact value; all pairs within [exact - tol, exact of the grown boxes + tol]. Returns the clear pairs'
    worst |error| / tol, printed before it is asserted."""
    got = np.asarray(got, np.float64)
    want, tol = e.want(kind)
    lo, hi = e.bounds(kind)
    assert got.shape == want.shape and np.isfinite(got).all(), label
    ratio = worst_ratio(got, want, tol, ~e.shell)
    out = (got < lo) | (got > hi)
    print("%s %s: %d pairs, %d overlapping, %d in the shell, clear pairs' worst error / tol %.3f, outside the bound %d"
          % (label, kind, got.size, (e.ov > 0).sum(), ((e.ov > 0) & e.shell).sum(), ratio, out.sum()))
    assert ratio <= 1.0, (label, kind, ratio)
    assert not out.any(), (label, kind, np.argwhere(out)[:5].tolist())
    return ratio


def iou_from_overlap(kind, a, b, so):
    """iou_bev_g / iou3d_g applied in float32, operation for operation, to a float32 overlap matrix `so`."""
    f32 = np.float32
    a, b, so = np.asarray(a, f32), np.asarray(b, f32), np.asarray(so, f32)
    sa, sb = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    if kind == "iou_bev":
        return so / np.maximum(sa[:, None] + sb[None, :] - so, f32(1e-8))
    amax, amin = a[:, 2] + a[:, 5] / f32(2), a[:, 2] - a[:, 5] / f32(2)
    bmax, bmin = b[:, 2] + b[:, 5] / f32(2), b[:, 2] - b[:, 5] / f32(2)
    oh = np.minimum(amax[:, None], bmax[None, :]) - np.maximum(amin[:, None], bmin[None, :])
    o3 = so * np.where(oh < 0, f32(0), oh)
    va, vb = sa * a[:, 5], sb * b[:, 5]
    return o3 / np.maximum(va[:, None] + vb[None, :] - o3, f32(1e-6))


def assert_zero_area_pairs(results, boxes, e, label="", ulps=0):
    """`results`: kind -> [n, n] float32 of `boxes` against themselves. What holds for the pairs with a box of no area
    (exact overlap 0), beyond assert_within:
      * clear of the margin shell they give 0 within tol;
      * in the shell the overlap is at most the area of the smaller box grown by the margin (+ tol). That is all the
        algorithm promises there: its 1e-2 corner margin counts the corners of a box smaller than the margin as inside
        a line or point box at the same place, and reports the small box's own area (1e-6 for the 1e-3 boxes);
      * the two IoUs are iou_bev_g / iou3d_g of that overlap, for every pair of the set: to the bit where every
        operation is correctly rounded (ulps = 0, the C restatement), within `ulps` float32 steps where the final
        division is not (the device's fp32 division is good to 2.5 ulp, so 4 with the roundings around it). So an IoU is wrong
        only as far as its overlap is, also where the all-pairs IoU bound says nothing because the denominator
        max(sa + sb - so, 1e-8) sits at its floor: a 1e-3 box against a line or point box gives so = 1e-6 over
        1e-8, BEV IoU 100, and 3-D IoU 1.2 - 1.6.
    Returns the (row, column, overlap, BEV IoU, 3-D IoU) of the pairs that are not 0."""
    flat = (e.a[:, 3] * e.a[:, 4] == 0)[:, None] | (e.b[:, 3] * e.b[:, 4] == 0)[None, :]
    assert flat.sum() > 1000 and np.all(e.ov[flat] == 0), label
    clear = flat & ~e.shell
    assert clear.sum() > 500, label
    for kind, got in results.items():
        assert np.all(np.abs(got[clear]) <= e.want(kind)[1][clear]), (label, kind)
    ga, gb = grown_area(e.a), grown_area(e.b)
    most = np.minimum(ga[:, None], gb[None, :]) + e.tol
    assert np.all(results["overlap"][flat] <= most[flat]), label
    for kind in ("iou_bev", "iou3d"):
        np.testing.assert_allclose(results[kind], iou_from_overlap(kind, boxes, boxes, results["overlap"]), rtol=ulps * 2.0 ** -23,
                                   atol=0, err_msg=label + " " + kind)
    found = [(int(i), int(j), float(results["overlap"][i, j]), float(results["iou_bev"][i, j]), float(results["iou3d"][i, j]))
             for i, j in np.argwhere(flat & (results["overlap"] != 0))]
    print("%s: %d of %d zero-area pairs are not 0 (%d of them in the shell); largest BEV IoU %.2f, 3-D IoU %.2f"
          % (label, len(found), flat.sum(), sum(bool(e.shell[i, j]) for i, j, *_ in found),
             max(f[3] for f in found) if found else 0, max(f[4] for f in found) if found else 0))
    return found


def grown_area(a, m=SHELL):
    return (a[:, 3] + 2 * m) * (a[:, 4] + 2 * m)


def turned(a):
    """The same rectangles with heading + pi (rounded to float32 like any input)."""
    t = np.array(a, np.float32)
    t[:, 6] += np.float32(np.pi)
    return t


def swapped(a):
    """The same rectangles as (dy, dx, heading + pi / 2)."""
    t = np.array(a, np.float32)[:, [0, 1, 2, 4, 3, 5, 6]]
    t[:, 6] += np.float32(np.pi / 2)
    return np.ascontiguousarray(t)


def lifted(a, dz):
    """The same boxes dz higher (the faces z +- dz / 2 round anew: Exact.want's height term grows with |z|)."""
    t = np.array(a, np.float32)
    t[:, 2] += np.float32(dz)
    return t


def assert_same_after_relabelling(run, kind, a, b, e, a2, b2, transpose=False, label=""):
    """run(kind, a2, b2) describes the same rectangles as run(kind, a, b) (transposed when the two sets changed
    places). The relabelled float32 boxes differ from the originals by the rounding of their new heading or z, so
    the result is held to its own exact value first, and to the original result within tol plus the exact values'
    own difference, on the pairs clear of the margin shell under both labellings."""
    e2 = Exact(a2, b2)
    got, got2 = np.asarray(run(kind, a, b), np.float64), np.asarray(run(kind, a2, b2), np.float64)
    assert_within(got2, e2, kind, label)
    (w, t), (w2, t2), shell2 = e.want(kind), e2.want(kind), e2.shell
    if transpose:
        got2, w2, t2, shell2 = got2.T, w2.T, t2.T, shell2.T
    clear = ~e.shell & ~shell2
    assert clear.sum() >= 0.9 * clear.size, label
    assert np.all(np.abs(got2 - got)[clear] <= (np.maximum(t, t2) + np.abs(w2 - w))[clear]), (label, kind)


def lidar_to_kitti_bev(a):
    """The (x, y, dx, dy, angle) float32 boxes of rotate_iou.py for lidar boxes: rbbox_to_corners turns a box by -angle
    (x' = cos * x + sin * y, y' = -sin * x + cos * y), so angle = -heading; centre and sizes carry over."""
    a = np.asarray(a, np.float32).reshape(-1, 7)
    return np.stack([a[:, 0], a[:, 1], a[:, 3], a[:, 4], -a[:, 6]], 1).astype(np.float32)


def lidar_to_kitti_camera(a):
    """The (x, y, z, l, h, w, ry) float64 camera boxes of d3_box_overlap for lidar boxes. Its BEV plane is columns
    (0, 2, 3, 5, 6) = (x, z, l, w, ry) and a box spans [y - h, y] on the downward y axis, so
    x_cam = x, z_cam = y, l = dx, w = dy, h = dz, ry = -heading, y_cam = -(z - dz / 2) (the bottom face)."""
    a = np.asarray(a, np.float32).reshape(-1, 7).astype(np.float64)
    return np.stack([a[:, 0], -(a[:, 2] - a[:, 5] / 2), a[:, 1], a[:, 3], a[:, 5], a[:, 4], -a[:, 6]], 1)


# ---- the sets ----------------------------------------------------------------------------------------------------------

PAIR_SHAPES = [(1, 1), (15, 63), (16, 64), (17, 65), (64, 1), (65, 129), (130, 257)]   # 16-row chunk, 64-row / 64-column block
SHIFTS = [0.0, 70.0]                                                                    # R ~ 12 .. 25 and R ~ 80 .. 95
MAX_SHELL_FRACTION = 0.35
NMS_SIZES = [63, 64, 65, 129, 200]
NMS_THR = 0.3
NMS_MARGIN = 0.02
KITTI_SHAPES = [(1, 1), (63, 65), (130, 40)]
KITTI_SHIFTS = [(0.0, 0.0), (70.0, 0.0)]        # near the origin and 70 m out along an axis (see kitti_set)
KITTI_EPS = 1e-3            # general position: 100 x the fp32 corner error at 80 m, far below any box size
_cache = {}


def _cached(fn):
    def wrapped(*key):
        if (fn.__name__, key) not in _cache:
            _cache[(fn.__name__, key)] = fn(*key)
        return _cache[(fn.__name__, key)]
    return wrapped


def _two_sets(seed, n, m, shift_x, shift_y):
    from cpd_amd.synthetic import random_boxes
    span = 1.6 * max(1.0, (n * m) ** 0.25)          # a constant density: >= 300 overlapping pairs from 65 x 129 on
    a, _ = random_boxes(seed, n, span=span)
    b, _ = random_boxes(seed + 500, m, span=span)
    for s in (a, b):
        s[:, 0] += np.float32(shift_x)
        s[:, 1] += np.float32(shift_y)
    return a, b


@_cached
def pair_set(n, m, shift):
    """(a [n, 7], b [m, 7], Exact) of random_boxes translated by (+shift, -shift): at least one overlapping pair (300 when
    n * m >= 65 * 129) and at most 35 % of the overlapping pairs in the margin shell."""
    need = 300 if n * m >= 65 * 129 else 1
    for seed in range(n + m, n + m + 64 * 7919, 7919):
        a, b = _two_sets(seed, n, m, shift, -shift)
        e = Exact(a, b)
        over = e.ov > 0
        if over.sum() >= need and (over & e.shell).sum() <= MAX_SHELL_FRACTION * over.sum():
            return a, b, e
    raise AssertionError("no set for %d x %d" % (n, m))


def zero_area_boxes(base):
    """Boxes with dx = 0, dy = 0, dx = dy = 0 (no area) and dz = 0 (no volume), rotated and axis-aligned, from `base` [>= 4, 7]."""
    z = np.repeat(np.asarray(base, np.float32)[:4], 2, axis=0)
    z[1::2, 6] = 0
    z[0:2, 3] = 0
    z[2:4, 4] = 0
    z[4:6, 3:5] = 0
    z[6:8, 5] = 0
    return z


@_cached
def degenerate_set(golden_dir):
    """(boxes, Exact(boxes, boxes), n_adv): the 84 adversarial boxes of tests/golden/iou_bev.npz and 8 zero-area / zero-height ones."""
    import os
    adv = np.load(os.path.join(golden_dir, "iou_bev.npz"))["adv"].astype(np.float32)
    boxes = np.concatenate([adv, zero_area_boxes(adv)], 0)
    return boxes, Exact(boxes, boxes), len(adv)


def greedy_nms(iou, thr):
    """Greedy scan over an IoU matrix of boxes in descending score order: kept row ids."""
    n = len(iou)
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if not dead[i]:
            keep.append(i)
            dead[i + 1:] |= iou[i, i + 1:] > thr
    return np.array(keep, np.int64)


@_cached
def nms_set(n, thr):
    """(boxes in descending score order, Exact): no pair has an exact IoU within NMS_MARGIN of thr, and thr lies outside
    every pair's [lo, hi] bound, so the margin shell cannot move a pair across the threshold."""
    from cpd_amd.synthetic import random_boxes
    for seed in range(n, n + 256 * 7919, 7919):
        b, s = random_boxes(seed, n, span=max(8.0, 0.36 * n))    # ~40 overlapping pairs: one seed in four is clean
        bs = np.ascontiguousarray(b[np.argsort(-s, kind="stable")])
        e = Exact(bs, bs)
        iou, _ = e.want("iou_bev")
        lo, hi = e.bounds("iou_bev")
        up = np.triu_indices(n, 1)
        if np.all(np.abs(iou[up] - thr) >= NMS_MARGIN) and np.all((hi[up] < thr) | (lo[up] > thr)):
            return bs, e
    raise AssertionError("no set for n=%d" % n)


@_cached
def kitti_set(n, m, shift_x, shift_y=0.0):
    """(a, b, Exact, general_position mask) for the rotate_iou.py overlap: at least 95 % of the overlapping pairs in
    general position. The far sets lie 70 m out along one axis: rotate_iou.py's line_segment_intersection multiplies
    absolute coordinates (A0 * B1 - B0 * A1), so its error grows with |x * y|, not with R -- see test_box_exact_ref."""
    for seed in range(3 * n + m, 3 * n + m + 64 * 7919, 7919):
        a, b = _two_sets(seed, n, m, shift_x, shift_y)
        e = Exact(a, b)
        gp = general_position(a, b, KITTI_EPS)
        over = e.ov > 0
        if over.any() and (over & gp).sum() >= 0.95 * over.sum():
            return a, b, e, gp
    raise AssertionError("no set for %d x %d" % (n, m))


def kitti_want(e, criterion, volume=False):
    """(exact, tolerance) [N, M] of rotate_iou_gpu_eval(boxes = a, query = b, criterion) (volume=False: -1 IoU, 0 over the
    QUERY's area, 1 over the box's area, 2 the intersection area) and of d3_box_overlap(a, b, criterion) (volume=True:
    -1 IoU, 0 over the BOX's volume, 1 over the query's volume, 2 intersection over itself: 1 where there is any)."""
    h = e.oh if volume else 1.0
    inter, tol = e.ov * h, e.tol * h
    za = (e.a[:, 3] * e.a[:, 4] * (e.a[:, 5] if volume else 1.0))[:, None] + 0 * inter
    zb = (e.b[:, 3] * e.b[:, 4] * (e.b[:, 5] if volume else 1.0))[None, :] + 0 * inter
    if criterion == -1:
        den = za + zb - inter
    elif criterion == 0:
        den = za if volume else zb
    elif criterion == 1:
        den = zb if volume else za
    elif volume:
        return (inter > 0).astype(np.float64), np.zeros_like(inter)
    else:
        den = np.ones_like(inter)
    return inter / den, tol / den
