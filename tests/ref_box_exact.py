"""Exact rotated-box overlap in numpy float64: the geometry the fp32 overlap kernels (csrc/box_geom.h, ke_rotate_iou in
csrc/kitti_eval.hip) are measured against. It shares nothing with either algorithm: corners from the box definition (dx
along the heading), a Sutherland-Hodgman clip of one rectangle by the other and the shoelace formula -- the clip and the
corner order are those of tests/ref_waymo_eval.py. Boxes are lidar boxes [N, 7] = (x, y, z, dx, dy, dz, heading); float32
inputs are taken at their float32 values.

Besides the overlaps it states what the tests may ask of an fp32 kernel:
  * tol_overlap: one fp32 ulp of corner displacement along both outlines, 2^-23 * R * (perimeter_a + perimeter_b), with R
    the largest |x| or |y| of the pair's corners;
  * in_shell / grown: box_geom.h counts a corner as inside a box when it is within 1e-2 of it per half-extent, so a pair
    with a corner in that shell may report up to the overlap of the grown boxes (the added points all lie in both grown
    boxes); 1.2e-2 is the kernel's 1e-2 plus fp32 slack;
  * general_position: pairs without shared corners, coincident or collinear edges (rotate_iou.py keeps the first 8
    candidate points, which is too few exactly there).
"""
import numpy as np

from ref_waymo_eval import _area, _clip, corners_bev

SHELL = 1.2e-2
IOU_EPS_BEV = 1e-8          # iou_bev_g:  so / max(sa + sb - so, 1e-8)
IOU_EPS_3D = 1e-6           # iou3d_g:    o3 / max(va + vb - o3, 1e-6)


def _f64(a):
    return np.asarray(a, dtype=np.float64).reshape(-1, 7)


def corners(a):
    """[N, 4, 2] counter-clockwise BEV corners."""
    a = _f64(a)
    return np.array([corners_bev(b) for b in a], dtype=np.float64).reshape(-1, 4, 2)


def overlap_bev(a, b):
    """[N, M] area of the intersection of the BEV rectangles. Only pairs whose circumscribed circles meet are clipped;
    a box with dx <= 0 or dy <= 0 has no area and overlaps nothing."""
    a, b = _f64(a), _f64(b)
    ca, cb = corners(a), corners(b)
    ra, rb = 0.5 * np.hypot(a[:, 3], a[:, 4]), 0.5 * np.hypot(b[:, 3], b[:, 4])
    dist = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
    near = dist <= ra[:, None] + rb[None, :] + 1e-9
    near &= ((a[:, 3] > 0) & (a[:, 4] > 0))[:, None] & ((b[:, 3] > 0) & (b[:, 4] > 0))[None, :]
    out = np.zeros((len(a), len(b)), dtype=np.float64)
    for i, j in zip(*np.nonzero(near)):
        out[i, j] = _area(_clip([tuple(p) for p in ca[i]], [tuple(p) for p in cb[j]]))
    return out


def areas(a):
    a = _f64(a)
    return a[:, 3] * a[:, 4]


def height_overlap(a, b):
    """[N, M] overlap of the z ranges, clamped at 0."""
    a, b = _f64(a), _f64(b)
    top = np.minimum((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None, :])
    bot = np.maximum((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None, :])
    return np.maximum(top - bot, 0.0)


def union_bev(a, b, ov):
    """The denominator of iou_bev_g for the intersection areas `ov`."""
    return np.maximum(areas(a)[:, None] + areas(b)[None, :] - ov, IOU_EPS_BEV)


def union_3d(a, b, ov):
    """The denominator of iou3d_g for the BEV intersection areas `ov`."""
    a, b = _f64(a), _f64(b)
    va, vb = areas(a) * a[:, 5], areas(b) * b[:, 5]
    return np.maximum(va[:, None] + vb[None, :] - ov * height_overlap(a, b), IOU_EPS_3D)


def iou_bev(a, b, ov=None):
    ov = overlap_bev(a, b) if ov is None else ov
    return ov / union_bev(a, b, ov)


def iou3d(a, b, ov=None):
    ov = overlap_bev(a, b) if ov is None else ov
    return ov * height_overlap(a, b) / union_3d(a, b, ov)


def grown(a, m=SHELL):
    """The same boxes with dx and dy increased by 2m."""
    g = _f64(a).copy()
    g[:, 3:5] += 2 * m
    return g


def _local(a, b):
    """Corners of b in the frames of a: (|rx|, |ry|) [N, M, 4] and a's half-extents [N, 1, 1] each."""
    a, b = _f64(a), _f64(b)
    cb = corners(b)
    c, s = np.cos(a[:, 6])[:, None, None], np.sin(a[:, 6])[:, None, None]
    px = cb[None, :, :, 0] - a[:, None, None, 0]
    py = cb[None, :, :, 1] - a[:, None, None, 1]
    return np.abs(c * px + s * py), np.abs(-s * px + c * py), a[:, 3][:, None, None] / 2, a[:, 4][:, None, None] / 2


def _shell_one_way(a, b, m):
    rx, ry, hx, hy = _local(a, b)
    inside = (rx <= hx + 1e-9) & (ry <= hy + 1e-9)            # a corner on the outline is not outside
    inside_grown = (rx < hx + m) & (ry < hy + m)
    return (inside_grown & ~inside).any(-1)


def in_shell(a, b, m=SHELL):
    """[N, M] bool: a corner of either box lies outside the other box but inside it grown by m per half-extent."""
    return _shell_one_way(a, b, m) | _shell_one_way(b, a, m).T


def _general_one_way(a, b, eps):
    rx, ry, hx, hy = _local(a, b)
    return ((np.abs(rx - hx) > eps) & (np.abs(ry - hy) > eps)).all(-1)


def general_position(a, b, eps):
    """[N, M] bool: no corner of one box lies within eps of an edge line of the other."""
    return _general_one_way(a, b, eps) & _general_one_way(b, a, eps).T


def tol_overlap(a, b):
    """[N, M] 2^-23 * R * (perimeter_a + perimeter_b), R the largest |x| or |y| of the pair's corners."""
    a, b = _f64(a), _f64(b)
    ra, rb = np.abs(corners(a)).max((1, 2)), np.abs(corners(b)).max((1, 2))
    pa, pb = 2 * (a[:, 3] + a[:, 4]), 2 * (b[:, 3] + b[:, 4])
    return 2.0 ** -23 * np.maximum(ra[:, None], rb[None, :]) * (pa[:, None] + pb[None, :])


class Exact:
    """Everything the tests compare a [N, M] overlap / IoU / 3-D IoU matrix with, computed once per pair of sets."""

    def __init__(self, a, b, m=SHELL):
        self.a, self.b = _f64(a), _f64(b)
        self.ov = overlap_bev(a, b)
        self.ov_grown = np.maximum(overlap_bev(grown(a, m), grown(b, m)), self.ov)
        self.tol = tol_overlap(a, b)
        self.shell = in_shell(a, b, m)
        self.oh = height_overlap(a, b)
        za, zb = (np.abs(s[:, 2]) + s[:, 5] / 2 for s in (self.a, self.b))
        self.tol_oh = 2.0 ** -23 * np.maximum(za[:, None], zb[None, :])     # the top and the bottom face, half an fp32 ulp each
        self.sum_bev = areas(a)[:, None] + areas(b)[None, :]
        self.sum_3d = (areas(a) * self.a[:, 5])[:, None] + (areas(b) * self.b[:, 5])[None, :]

    def want(self, kind):
        """(exact, tolerance) of `kind` in 'overlap', 'iou_bev', 'iou3d'; the IoU tolerance is the overlap's over the
        exact union. The 3-D IoU's intersection is area x height overlap, the latter a difference of two fp32 faces
        z +- dz / 2: its tolerance is (tol x height overlap + area x 2^-23 max|face|) over the union volume. The face
        term is small beside the first (faces of 2 - 3 m against R >= 12) except where two boxes barely overlap in
        height: tol x height overlap vanishes there while the faces' rounding does not. The sets at rest do not need it
        (the restatement's worst ratio without it: 0.37 random, 0.65 degenerate); the same boxes lifted by 1 m do
        (1.005 on the 65 x 129 set at the origin, on a pair with a small height overlap), and it is kept for them."""
        if kind == "overlap":
            return self.ov, self.tol
        if kind == "iou_bev":
            u = np.maximum(self.sum_bev - self.ov, IOU_EPS_BEV)
            return self.ov / u, self.tol / u
        u = np.maximum(self.sum_3d - self.ov * self.oh, IOU_EPS_3D)
        return self.ov * self.oh / u, (self.tol * self.oh + self.tol_oh * self.ov) / u

    def bounds(self, kind):
        """(lo, hi) for every pair: exact(a, b) - tol <= got <= exact(grown a, grown b) + tol, carried through the
        kernel's own expression for `kind` (the areas and volumes in its denominator are those of a and b)."""
        lo, tol = self.want(kind)
        if kind == "overlap":
            return lo - tol, self.ov_grown + tol
        most = self.ov_grown + self.tol                 # the IoU expressions grow with the overlap they are given
        if kind == "iou_bev":
            return lo - tol, most / np.maximum(self.sum_bev - most, IOU_EPS_BEV)
        most = most * (self.oh + self.tol_oh)
        return lo - tol, most / np.maximum(self.sum_3d - most, IOU_EPS_3D)


def worst_ratio(got, want, tol, mask):
    """max over `mask` of |got - want| / tol (0 when the mask is empty; a pair with tol = 0 must be met exactly)."""
    err = np.abs(np.asarray(got, np.float64) - want)[mask]
    t = tol[mask]
    if not err.size:
        return 0.0
    return float(np.where(err == 0, 0.0, err / np.where(t > 0, t, np.finfo(np.float64).tiny)).max())
