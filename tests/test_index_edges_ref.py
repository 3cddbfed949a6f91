"""The numpy restatements of tests/ref_index_edges.py against an independent source, bit for bit: the C oracle where it has the
operation (rulebooks, output set, NCHW densify, output shape), a brute-force loop over rows written out here where it has not
(row orders, tap masks, channels-last layouts, the dense 2-D table). Every site-set generator of the GPU edge suite runs here at its
smallest size, against its definition cell by cell, so the GPU file trusts nothing unchecked. CPU only."""
import itertools

import numpy as np
import pytest

import ref_index_edges as R

SMALL = [(1, [1, 1, 1]), (1, [1, 1, 65]), (2, [2, 3, 5]), (3, [5, 2, 31]), (1, [3, 4, 64])]


def _cases():
    """(batch, shape, ksize, stride, pad) -- a few dozen, anisotropic ones included; every one has a positive output shape"""
    rng = np.random.default_rng(11)
    out = [(2, [4, 6, 7], [3, 3, 3], [1, 1, 1], [1, 1, 1]), (1, [5, 8, 9], [3, 3, 3], [2, 2, 2], [1, 1, 1]),
           (2, [5, 8, 9], [3, 3, 3], [2, 2, 2], [0, 1, 1]), (1, [3, 5, 70], [1, 1, 32], [1, 1, 1], [0, 0, 16]),
           (1, [6, 3, 40], [3, 1, 5], [2, 1, 3], [0, 0, 2]), (1, [2, 9, 20], [1, 7, 7], [1, 3, 3], [0, 3, 3])]
    while len(out) < 36:
        shape = [int(v) for v in rng.integers(1, 9, 3)]
        k = [int(v) for v in rng.integers(1, 6, 3)]
        s = [int(v) for v in rng.integers(1, 4, 3)]
        p = [int(rng.integers(0, kk)) for kk in k]
        if min(R.out_shape(shape, k, s, p)) > 0:
            out.append((int(rng.integers(1, 4)), shape, k, s, p))
    return out


CASES = _cases()


def _sites(batch, shape, seed, frac=0.4):
    q = R.gen_random(frac, seed)(batch, shape)
    return R.shuffled(q, seed) if len(q) else q


@pytest.mark.parametrize("case", range(len(CASES)))
def test_tables_and_output_set_against_the_oracle(oracle, case):
    batch, shape, k, s, p = CASES[case]
    idx = _sites(batch, shape, case)
    assert oracle.conv_out_shape(shape, k, s, p) == R.out_shape(shape, k, s, p)
    lut = R.lookup(idx, batch, shape)
    out = R.outset(idx, batch, shape, k, s, p)
    np.testing.assert_array_equal(out, oracle.conv_outset(idx, batch, shape, k, s, p).reshape(-1, 4))
    np.testing.assert_array_equal(R.conv_table(lut, out, k, s, p), oracle.conv_rulebook(idx, out, batch, shape, k, s, p))
    ko = [kk | 1 for kk in k]                                        # sub-manifold kernels are odd
    np.testing.assert_array_equal(R.subm_table(lut, idx, ko), oracle.subm_rulebook(idx, batch, shape, ko))


def test_lookup_rank_map_and_ignored_rows():
    batch, shape = 2, [3, 4, 5]
    good = _sites(batch, shape, 5)
    bad = np.array([[-1, 0, 0, 0], [2, 0, 0, 0], [0, -1, 0, 0], [0, 3, 0, 0], [0, 0, -1, 0], [0, 0, 4, 0], [0, 0, 0, -1], [0, 0, 0, 5]], np.int32)
    idx = np.concatenate([bad[:4], good[:7], bad[4:], good[7:]])
    lut = R.lookup(idx, batch, shape)
    want = np.full(lut.shape, -1, np.int64)
    for i, q in enumerate(idx):                                      # brute force: the definition, row by row
        if 0 <= q[0] < batch and all(0 <= q[1 + d] < shape[d] for d in range(3)):
            want[tuple(q)] = i
    np.testing.assert_array_equal(lut, want)
    assert (lut >= 0).sum() == len(good)
    np.testing.assert_array_equal(R.canonical(idx, batch, shape), np.array(sorted(map(tuple, good)), np.int32))
    # a rank -> row map: the site of canonical rank r gets row map[r]
    rmap = np.random.default_rng(2).permutation(len(good)) + 100
    lut2 = R.lookup(idx, batch, shape, rmap)
    for r, q in enumerate(sorted(map(tuple, good))):
        assert lut2[q] == rmap[r]
    assert ((lut2 >= 0) == (lut >= 0)).all()


def test_tapmask_and_pattern_brute_force():
    rng = np.random.default_rng(4)
    for kv, n in [(27, 1), (27, 16), (27, 17), (9, 63), (32, 65), (3, 33)]:
        tab = np.where(rng.random((kv, n)) < 0.2, rng.integers(0, 50, (kv, n)), -1).astype(np.int32)
        tab[:, n // 2] = -1                                          # a row without taps
        want_p = [sum(1 << t for t in range(kv) if tab[t, j] >= 0) for j in range(n)]
        np.testing.assert_array_equal(R.row_pattern(tab), np.array(want_p, np.uint32))
        want_m = [0] * ((n + 15) // 16)
        for j in range(n):
            want_m[j // 16] |= want_p[j]
        np.testing.assert_array_equal(R.tapmask(tab), np.array(want_m, np.uint32))
    with pytest.raises(AssertionError):
        R.tapmask(np.zeros((45, 3), np.int32))


def test_tap_order_brute_force():
    rng = np.random.default_rng(6)
    for n, chunk in [(1, 4), (7, 4), (8, 4), (9, 4), (40, 16), (300, 128)]:
        pat = rng.choice(np.array([0, 1, 0x2000, 0x7ffffff, 0x7fffffe, 0xf8002000], np.uint32), n)    # bits 27.. are not part of the key
        n2o, o2n = R.tap_order(pat, chunk)
        want = []
        for c0 in range(0, n, chunk):
            want += sorted(range(c0, min(n, c0 + chunk)), key=lambda j: int(pat[j]) & 0x7ffffff)       # sorted() is stable
        np.testing.assert_array_equal(n2o, want)
        np.testing.assert_array_equal(o2n[n2o], np.arange(n))


def test_brick_order_brute_force():
    batch, shape = 2, [2, 9, 20]
    q = R.gen_random(0.5, 3)(batch, shape)
    for by, bx in [(8, 8), (4, 16), (1, 1), (64, 64)]:
        want = sorted(range(len(q)), key=lambda j: (q[j][0], q[j][1], q[j][2] // by, q[j][3] // bx, q[j][2], q[j][3]))
        np.testing.assert_array_equal(R.brick_order(q, shape, by, bx), want)
    np.testing.assert_array_equal(R.brick_order(q, shape, 1, 1), np.arange(len(q)))      # 1 x 1 bricks: canonical order
    np.testing.assert_array_equal(R.brick_order(q, shape, 64, 64), np.arange(len(q)))    # one brick per plane: canonical order
    # the composed order: brick positions, then a stable pattern sort inside every tile
    lut = R.lookup(q, batch, shape)
    pat = R.row_pattern(R.subm_table(lut, q, [3, 3, 3]))
    for tile in (128, 256):
        out, n2o, o2n = R.brick_tile_order(q, batch, shape, 8, 8, tile)
        p2r = R.brick_order(q, shape, 8, 8)
        want = []
        for c0 in range(0, len(q), tile):
            want += sorted(p2r[c0:c0 + tile], key=lambda j: int(pat[j]) & 0x7ffffff)
        np.testing.assert_array_equal(n2o, want)
        np.testing.assert_array_equal(out, q[n2o])
        np.testing.assert_array_equal(o2n[n2o], np.arange(len(q)))


def _payload(n, c, seed):
    f = np.random.default_rng(seed).integers(1, 2 ** 32, (n, c), dtype=np.uint64).astype(np.uint32)
    f.reshape(-1)[:3] = [0x80000000, 0x7fc12345, 0x00000001][:f.size]                  # -0.0, a NaN with a payload, a denormal
    return f


@pytest.mark.parametrize("c", [1, 3, 4])
def test_densify_layouts(oracle, c):
    batch, shape = 2, [3, 4, 5]
    D, H, W = shape
    idx = _sites(batch, shape, 9)
    f = _payload(len(idx), c, c)
    # NCHW against the oracle on finite values (the oracle moves floats: NaN payloads are compared by the loops below instead)
    fv = np.random.default_rng(c).standard_normal((len(idx), c)).astype(np.float32)
    np.testing.assert_array_equal(R.densify_nchw(fv, idx, batch, shape), oracle.densify(fv, idx, batch, shape).view(np.uint32))
    nchw, nhwc, cd = R.densify_nchw(f, idx, batch, shape), R.densify_nhwc(f, idx, batch, shape), R.densify_nhwc_cd(f, idx, batch, shape)
    w_nchw, w_nhwc, w_cd = np.zeros((batch, c * D, H, W), np.uint32), np.zeros((batch, H, W, D * c), np.uint32), np.zeros((batch, H, W, c * D), np.uint32)
    for i, (b, z, y, x) in enumerate(idx):
        for ch in range(c):
            w_nchw[b, ch * D + z, y, x] = f[i, ch]
            w_nhwc[b, y, x, z * c + ch] = f[i, ch]
            w_cd[b, y, x, ch * D + z] = f[i, ch]
    np.testing.assert_array_equal(nchw, w_nchw)
    np.testing.assert_array_equal(nhwc, w_nhwc)
    np.testing.assert_array_equal(cd, w_cd)
    np.testing.assert_array_equal(cd, nchw.transpose(0, 2, 3, 1))                          # the same channel order, channels last
    # rows into a map that is not zero, then clear: only the sites' rows change
    base = np.full((batch, H, W, D * c), 0x11111111, np.uint32)
    rows = R.densify_nhwc_rows(base, f, idx, shape)
    occ = nhwc != 0
    np.testing.assert_array_equal(rows[occ], nhwc[occ])
    cleared = R.densify_nhwc_clear(rows, idx, c, shape)
    touched = np.zeros_like(occ)
    for b, z, y, x in idx:
        touched[b, y, x, z * c:(z + 1) * c] = True
    assert (cleared[touched] == 0).all() and (cleared[~touched] == 0x11111111).all()
    np.testing.assert_array_equal(R.densify_nhwc_clear(nhwc, idx, c, shape), np.zeros_like(nhwc))


def test_conv2d_table_brute_force():
    for batch, h, w, kh, kw, s, p in [(1, 1, 1, 1, 1, 1, 0), (2, 5, 7, 3, 3, 1, 1), (1, 6, 9, 3, 3, 2, 1), (3, 4, 4, 2, 2, 2, 0), (1, 7, 5, 5, 3, 3, 2)]:
        ho, wo = (h + 2 * p - kh) // s + 1, (w + 2 * p - kw) // s + 1
        want = np.full((kh * kw, batch * ho * wo), -1, np.int32)
        for b, y, x, ky, kx in itertools.product(range(batch), range(ho), range(wo), range(kh), range(kw)):
            iy, ix = y * s - p + ky, x * s - p + kx
            if 0 <= iy < h and 0 <= ix < w:
                want[ky * kw + kx, (b * ho + y) * wo + x] = (b * h + iy) * w + ix
        np.testing.assert_array_equal(R.conv2d_table(batch, h, w, kh, kw, s, p), want)


# ------------------------------------------------------------------------------------------------ the generators, cell by cell
def _define(name, b, z, y, x, batch, shape):
    D, H, W = shape
    key = ((b * D + z) * H + y) * W + x
    cells = batch * D * H * W
    if name == "single":
        return (b, z, y, x) == (batch - 1, D // 2, H // 2, W // 2)
    if name == "empty":
        return False
    if name == "full":
        return True
    if name == "checker":
        return (b + z + y + x) % 2 == 0
    if name == "lines":
        return ((b * D + z) * H + y) % 3 == 0
    if name == "box":
        return all(e < 3 or 1 <= v < e - 1 for v, e in zip((z, y, x), shape))
    if name == "word_edges":
        return key in (0, cells - 1) or (key >= 63 and key % 64 in (63, 0, 1))    # 64 k - 1, 64 k, 64 k + 1 for k >= 1
    raise KeyError(name)


@pytest.mark.parametrize("name", list(R.GENERATORS))
@pytest.mark.parametrize("grid", range(len(SMALL)))
def test_generators(oracle, name, grid):
    batch, shape = SMALL[grid]
    q = R.GENERATORS[name](batch, shape)
    assert q.dtype == np.int32 and q.shape[1:] == (4,)
    assert R.valid_rows(q, batch, shape).all()
    np.testing.assert_array_equal(q, R.canonical(q, batch, shape))                          # canonical order, no duplicates
    assert len(np.unique(q, axis=0)) == len(q)
    if not name.startswith("random"):
        want = [c for c in itertools.product(range(batch), *[range(e) for e in shape]) if _define(name, *c, batch, shape)]
        np.testing.assert_array_equal(q, np.array(want, np.int32).reshape(-1, 4))
    else:
        cells = batch * int(np.prod(shape))
        frac = 0.05 if name == "random5" else 0.5
        assert abs(len(q) - frac * cells) <= 4 * np.sqrt(cells) + 1
        np.testing.assert_array_equal(q, R.GENERATORS[name](batch, shape))                  # deterministic
    # and through the tables, canonical and shuffled, against the oracle
    for lst in (q, R.shuffled(q)):
        lut = R.lookup(lst, batch, shape)
        np.testing.assert_array_equal(R.subm_table(lut, lst, [3, 3, 3]), oracle.subm_rulebook(lst, batch, shape, [3, 3, 3]).reshape(27, -1))
        out = R.outset(lst, batch, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1])
        np.testing.assert_array_equal(out, oracle.conv_outset(lst, batch, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1]).reshape(-1, 4))
        np.testing.assert_array_equal(R.conv_table(lut, out, [3, 3, 3], [2, 2, 2], [1, 1, 1]),
                                      oracle.conv_rulebook(lst, out, batch, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1]).reshape(27, -1))


def test_box_has_every_neighbour_pattern_class():
    """the property the GPU suite leans on: interior rows of a box have all 27 neighbours -- the padding key of the tap sort"""
    batch, shape = 1, [5, 6, 7]
    q = R.gen_box(batch, shape)
    pat = R.row_pattern(R.subm_table(R.lookup(q, batch, shape), q, [3, 3, 3]))
    counts = np.array([bin(int(p)).count("1") for p in pat])
    assert (pat == 0x7ffffff).sum() == 1 * 2 * 3 and set(counts) == {8, 12, 18, 27}       # corners, edges, faces, interior
