"""Plain numpy restatements (int64, no torch, no GPU) of what cpd_amd/csrc/site_index.hip builds: the coordinate -> row lookup, the
sub-manifold and strided rulebooks with their 16-row tap masks, the active output set of a strided conv, the tap-pattern and brick
row orders, the densify layouts and the dense 2-D table -- each on a DENSE lookup array of the grid, no bitmap, no prefix, no
words. tests/test_gpu_index_edges.py compares the HIP builders with them bit for bit; tests/test_index_edges_ref.py checks them
against the C oracle and against brute-force loops on the CPU.

Site lists are int32 [n, 4] rows (b, z, y, x); "canonical" order is ascending (b, z, y, x). The deterministic site-set generators
of both test files live here too (GENERATORS)."""
import numpy as np

PAD_KEY = 0x7ffffff                  # 27 pattern bits: the sort key of the tap orders


# ------------------------------------------------------------------------------------------------ lookup and tables
def valid_rows(indices, batch, shape):
    """which rows of a list lie inside the grid (the others are ignored by every builder)"""
    q = np.asarray(indices, np.int64).reshape(-1, 4)
    hi = np.array([batch, shape[0], shape[1], shape[2]], np.int64)
    return ((q >= 0) & (q < hi)).all(1)


def canonical(indices, batch, shape):
    """the in-grid rows of a list in ascending (b, z, y, x) order, int32 [m, 4]"""
    q = np.asarray(indices, np.int64).reshape(-1, 4)
    q = q[valid_rows(q, batch, shape)]
    return q[np.lexsort((q[:, 3], q[:, 2], q[:, 1], q[:, 0]))].astype(np.int32)


def lookup(indices, batch, shape, rank_to_row=None):
    """Dense [batch, D, H, W] int64 array: the row id of the site at a cell, -1 where there is none. Without a map the row id is
    the site's position in `indices` (out-of-grid rows take a position but own no cell); with `rank_to_row` it is
    rank_to_row[rank], rank = the site's place in canonical order ("canonical" = np.arange)."""
    q = np.asarray(indices, np.int64).reshape(-1, 4)
    lut = np.full((batch, shape[0], shape[1], shape[2]), -1, np.int64)
    rows = np.flatnonzero(valid_rows(q, batch, shape))
    lut[q[rows, 0], q[rows, 1], q[rows, 2], q[rows, 3]] = rows
    if rank_to_row is not None:
        occ = lut.reshape(-1) >= 0
        lut.reshape(-1)[occ] = np.asarray(rank_to_row, np.int64)[:occ.sum()]      # flat order of the array IS canonical order
    return lut


def out_shape(in_shape, ksize, stride, pad):
    return [(in_shape[d] + 2 * pad[d] - ksize[d]) // stride[d] + 1 for d in range(3)]


def conv_table(lut, out_indices, ksize, stride, pad):
    """nbr [kv, n_out] int32: nbr[t, j] = row at input cell out[j] * stride - pad + tap t (taps in (z, y, x) order), -1 outside the
    grid or where there is no site."""
    o = np.asarray(out_indices, np.int64).reshape(-1, 4)
    _, D, H, W = lut.shape
    nbr = np.full((ksize[0] * ksize[1] * ksize[2], o.shape[0]), -1, np.int64)
    t = 0
    for tz in range(ksize[0]):
        for ty in range(ksize[1]):
            for tx in range(ksize[2]):
                z = o[:, 1] * stride[0] - pad[0] + tz
                y = o[:, 2] * stride[1] - pad[1] + ty
                x = o[:, 3] * stride[2] - pad[2] + tx
                ok = (z >= 0) & (z < D) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
                nbr[t, ok] = lut[o[ok, 0], z[ok], y[ok], x[ok]]
                t += 1
    return nbr.astype(np.int32)


def subm_table(lut, indices, ksize):
    return conv_table(lut, indices, ksize, [1, 1, 1], [k // 2 for k in ksize])


def outset(indices, batch, in_shape, ksize, stride, pad):
    """canonical (b, z, y, x) list of the output cells o with an input site at o * stride - pad + t for some tap t"""
    q = np.asarray(indices, np.int64).reshape(-1, 4)
    os_ = out_shape(in_shape, ksize, stride, pad)
    mark = np.zeros((batch, os_[0], os_[1], os_[2]), bool)
    for tz in range(ksize[0]):
        for ty in range(ksize[1]):
            for tx in range(ksize[2]):
                n = q[:, 1:] + np.array(pad, np.int64) - np.array([tz, ty, tx], np.int64)
                ok = (n >= 0).all(1) & (n % np.array(stride, np.int64) == 0).all(1)
                n = n // np.array(stride, np.int64)
                ok &= (n < np.array(os_, np.int64)).all(1)
                mark[q[ok, 0], n[ok, 0], n[ok, 1], n[ok, 2]] = True
    return np.argwhere(mark).astype(np.int32).reshape(-1, 4)


def row_pattern(table):
    """uint32 [n]: bit t set iff row j has tap t (t < 32)"""
    kv, n = table.shape
    pat = np.zeros(n, np.int64)
    for t in range(min(kv, 32)):
        pat |= (table[t] >= 0).astype(np.int64) << t
    return pat.astype(np.uint32)


def tapmask(table):
    """uint32 [(n + 15) // 16]: bit t of word g set iff some row of the 16-row group g has tap t (kv <= 32)"""
    kv, n = table.shape
    assert kv <= 32
    pat = row_pattern(table).astype(np.int64)
    out = np.zeros((n + 15) // 16, np.int64)
    for j in range(n):
        out[j // 16] |= pat[j]
    return out.astype(np.uint32)


# ------------------------------------------------------------------------------------------------ row orders
def tap_order(pattern, chunk):
    """(new_to_old, old_to_new) int32 [n]: every chunk of `chunk` consecutive rows sorted by pattern & 0x7ffffff, stably"""
    key = np.asarray(pattern, np.int64) & PAD_KEY
    n = key.shape[0]
    n2o = np.empty(n, np.int64)
    for c0 in range(0, n, chunk):
        n2o[c0:c0 + chunk] = c0 + np.argsort(key[c0:c0 + chunk], kind="stable")
    o2n = np.empty(n, np.int64)
    o2n[n2o] = np.arange(n)
    return n2o.astype(np.int32), o2n.astype(np.int32)


tile_order = tap_order               # the same sort inside every 128- or 256-row tile of a brick order


def brick_order(indices, shape, by, bx):
    """position -> row of a CANONICAL list sorted by (b, z, y // by, x // bx, y, x)"""
    q = np.asarray(indices, np.int64).reshape(-1, 4)
    return np.lexsort((q[:, 3], q[:, 2], q[:, 3] // bx, q[:, 2] // by, q[:, 1], q[:, 0])).astype(np.int32)


def brick_tile_order(indices, batch, shape, by, bx, tile):
    """What cpd_order_rows_bricks returns for a canonical list: (indices in the new order, new_to_old, old_to_new) -- brick order,
    then inside every tile of that order a stable sort by the rows' 3 x 3 x 3 sub-manifold neighbour pattern."""
    q = np.asarray(indices, np.int32).reshape(-1, 4)
    p2r = brick_order(q, shape, by, bx).astype(np.int64)
    pat = row_pattern(subm_table(lookup(q, batch, shape), q, [3, 3, 3]))
    local, _ = tile_order(pat[p2r], tile)
    n2o = p2r[local]
    o2n = np.empty(q.shape[0], np.int64)
    o2n[n2o] = np.arange(q.shape[0])
    return q[n2o], n2o.astype(np.int32), o2n.astype(np.int32)


# ------------------------------------------------------------------------------------------------ densify (payload BITS: uint32)
def _bits(feat):
    f = np.ascontiguousarray(feat)
    return f.view(np.uint32) if f.dtype != np.uint32 else f


def densify_nchw(feat, indices, batch, shape):
    """[batch, C * D, H, W] uint32, channel c * D + z"""
    f, q = _bits(feat), np.asarray(indices, np.int64).reshape(-1, 4)
    D, H, W = shape
    c = f.shape[1]
    out = np.zeros((batch, c, D, H, W), np.uint32)
    for i in range(q.shape[0]):
        out[q[i, 0], :, q[i, 1], q[i, 2], q[i, 3]] = f[i]
    return out.reshape(batch, c * D, H, W)


def densify_nhwc_rows(dense, feat, indices, shape):
    """the rows of `feat` scattered into a copy of the [batch, H, W, D * C] uint32 map `dense`, channel z * C + c"""
    f, q = _bits(feat), np.asarray(indices, np.int64).reshape(-1, 4)
    c = f.shape[1]
    out = _bits(dense).copy().reshape(-1, shape[1], shape[2], shape[0], c)
    for i in range(q.shape[0]):
        out[q[i, 0], q[i, 2], q[i, 3], q[i, 1], :] = f[i]
    return out.reshape(-1, shape[1], shape[2], shape[0] * c)


def densify_nhwc_clear(dense, indices, c, shape):
    """the same rows of a copy of `dense` set to zero bits"""
    return densify_nhwc_rows(dense, np.zeros((np.asarray(indices).reshape(-1, 4).shape[0], c), np.uint32), indices, shape)


def densify_nhwc(feat, indices, batch, shape):
    """[batch, H, W, D * C] uint32, channel z * C + c"""
    c = _bits(feat).shape[1]
    return densify_nhwc_rows(np.zeros((batch, shape[1], shape[2], shape[0] * c), np.uint32), feat, indices, shape)


def densify_nhwc_cd(feat, indices, batch, shape):
    """[batch, H, W, C * D] uint32, channel c * D + z (the reference's channel order on channels-last pixels)"""
    f, q = _bits(feat), np.asarray(indices, np.int64).reshape(-1, 4)
    c = f.shape[1]
    out = np.zeros((batch, shape[1], shape[2], c, shape[0]), np.uint32)
    for i in range(q.shape[0]):
        out[q[i, 0], q[i, 2], q[i, 3], :, q[i, 1]] = f[i]
    return out.reshape(batch, shape[1], shape[2], c * shape[0])


def conv2d_table(batch, h, w, kh, kw, stride, pad):
    """nbr [kh * kw, batch * ho * wo] int32 of a dense 2-D conv: rows are pixels (b, y, x) in order"""
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    b, y, x = [a.reshape(-1) for a in np.meshgrid(np.arange(batch), np.arange(ho), np.arange(wo), indexing="ij")]
    nbr = np.full((kh * kw, b.size), -1, np.int64)
    for ky in range(kh):
        for kx in range(kw):
            iy, ix = y * stride - pad + ky, x * stride - pad + kx
            ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
            nbr[ky * kw + kx, ok] = ((b * h + iy) * w + ix)[ok]
    return nbr.astype(np.int32)


# ------------------------------------------------------------------------------------------------ site-set generators
def from_keys(keys, batch, shape):
    """linear cell keys ((b * D + z) * H + y) * W + x -> canonical int32 [n, 4]"""
    k = np.unique(np.asarray(keys, np.int64))
    D, H, W = shape
    return np.stack([k // (D * H * W), k // (H * W) % D, k // W % H, k % W], 1).astype(np.int32)


def _cells(batch, shape):
    return batch * shape[0] * shape[1] * shape[2]


def gen_empty(batch, shape):
    return np.zeros((0, 4), np.int32)


def gen_single(batch, shape):
    return np.array([[batch - 1, shape[0] // 2, shape[1] // 2, shape[2] // 2]], np.int32)


def gen_full(batch, shape):
    return from_keys(np.arange(_cells(batch, shape)), batch, shape)


def gen_checker(batch, shape):
    q = gen_full(batch, shape).astype(np.int64)
    return q[q.sum(1) % 2 == 0].astype(np.int32)


def gen_lines(batch, shape):
    """whole x-lines, every third line (b, z, y) of the grid"""
    q = gen_full(batch, shape).astype(np.int64)
    line = (q[:, 0] * shape[0] + q[:, 1]) * shape[1] + q[:, 2]
    return q[line % 3 == 0].astype(np.int32)


def gen_box(batch, shape):
    """a dense box one cell inside every face the grid is thick enough to have (an axis of extent < 3 is filled), in every batch:
    interior rows have all their neighbours; faces, edges and corners give the other patterns"""
    q = gen_full(batch, shape).astype(np.int64)
    keep = np.ones(q.shape[0], bool)
    for d in range(3):
        if shape[d] >= 3:
            keep &= (q[:, 1 + d] >= 1) & (q[:, 1 + d] < shape[d] - 1)
    return q[keep].astype(np.int32)


def gen_word_edges(batch, shape):
    """cells at linear keys 64 k - 1, 64 k, 64 k + 1, and the first and last cell of the grid"""
    cells = _cells(batch, shape)
    k = np.arange(64, cells + 64, 64)
    keys = np.concatenate([[0, cells - 1], k - 1, k, k + 1])
    return from_keys(keys[(keys >= 0) & (keys < cells)], batch, shape)


def gen_random(frac, seed=0):
    def gen(batch, shape):
        cells = _cells(batch, shape)
        rng = np.random.default_rng(seed + cells)
        return from_keys(np.flatnonzero(rng.random(cells) < frac), batch, shape)
    return gen


GENERATORS = {"single": gen_single, "empty": gen_empty, "full": gen_full, "checker": gen_checker, "lines": gen_lines, "box": gen_box,
              "word_edges": gen_word_edges, "random5": gen_random(0.05), "random50": gen_random(0.5)}


def shuffled(indices, seed=1):
    q = np.asarray(indices, np.int32).reshape(-1, 4)
    return q[np.random.default_rng(seed).permutation(q.shape[0])]
