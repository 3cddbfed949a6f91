"""The table builders of cpd_amd/csrc/site_index.hip at their edges: the occupancy bitmap and its popcount prefix, the sub-manifold
and strided rulebooks with their tap masks, the output set of a strided conv, the tap-pattern and brick row orders, the
chunk-ordered rulebook and the densify layouts -- against the plain numpy restatements of tests/ref_index_edges.py (checked on the
CPU by tests/test_index_edges_ref.py), bit for bit: these are integer tables and copied bits, there is no tolerance anywhere.

The C entry points are called through cpd_amd._lib so that every output starts as a fixed bit pattern with guard elements behind
its end, and every index buffer as a non-zero byte pattern: stale memory cannot pass for a table entry or a prefix, and whatever
a call has no business writing must come back untouched. Sections A - I follow the builders' branch points: bitmap word geometry,
scan tiles, row counts around 16 / 64 / 256, strided output sets, the tap sort's radix passes and padding key, the 4096-row
chunk rulebook, bricks clipped by the grid (and the index the batched voxelizer leaves behind), the densify layouts, index building."""

import numpy as np
import pytest
import torch

import ref_index_edges as R
from cpd_amd import _lib

gpu = pytest.mark.gpu

OK, ARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
PATTERN = 0x5A5A5A5A                 # what every output holds before a call
GUARD = 64                           # guard elements behind every output
POISON = 0xA5                        # the byte index buffers and workspaces hold before a builder writes into them
SCAN_TILE = 4096                     # words per scan block (common.h)
ONE = [1, 1, 1]


def L():
    return _lib.lib()


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def fenced(n):
    """int32 [n + GUARD] of PATTERN"""
    return torch.full((int(n) + GUARD,), PATTERN, dtype=torch.int32, device="cuda")


def host(t, n=None, shape=None, dtype=np.int32):
    """the first n elements of a fenced tensor, after asserting that everything behind them still holds the pattern"""
    a = t.cpu().numpy()
    n = a.size - GUARD if n is None else n
    assert (a[n:] == PATTERN).all(), "wrote past the end of an output"
    a = a[:n].view(dtype)
    return a.reshape(shape) if shape is not None else a


def untouched(t):
    return bool((t == PATTERN).all().item())


def poison(nbytes):
    return torch.full((int(nbytes) + 256,), POISON, dtype=torch.uint8, device="cuda")


def a256(x):
    return (x + 255) // 256 * 256


class Index:
    """A site index in a poisoned buffer with 256 guard bytes behind it; the layout of site_index_layout.h restated."""

    def __init__(self, batch, shape, cap):
        self.batch, self.shape, self.cap = batch, list(shape), cap
        self.cells = batch * shape[0] * shape[1] * shape[2]
        self.words = (self.cells + 63) // 64
        self.nb = max(1, (self.words + SCAN_TILE - 1) // SCAN_TILE)
        self.o_bitmap = 256
        self.o_base = self.o_bitmap + a256(self.words * 8)
        self.o_bsum = self.o_base + a256(self.words * 4)
        self.o_perm = self.o_bsum + a256((self.nb + 1) * 4)
        self.bytes = self.o_perm + a256(max(cap, 1) * 4)
        assert self.bytes == L().cpd_index_bytes(batch, _lib.iarr(shape), cap)
        self.buf = poison(self.bytes)
        self.order = None

    def ptr(self):
        return _lib.ptr(self.buf)

    def build(self, idx):
        self.list = dev(idx.reshape(-1, 4))
        n = self.list.shape[0]
        assert n <= max(self.cap, 1)
        return L().cpd_index_build(_lib.ptr(self.list), n, self.batch, _lib.iarr(self.shape), self.ptr(), self.bytes, _lib.stream())

    def set_order(self, rank_to_row):
        self.order = None if rank_to_row is None else dev(rank_to_row)
        assert L().cpd_index_set_order(self.ptr(), _lib.ptr(self.order), _lib.stream()) == OK

    def part(self, off, count, dtype):
        nbytes = count * np.dtype(dtype).itemsize
        return self.buf[off:off + nbytes].cpu().numpy().view(dtype)

    def guard_ok(self):
        return bool((self.buf[self.bytes:] == POISON).all().item())

    def check(self, idx, n_perm=None):
        """bitmap, prefix and own rank -> row map of a cpd_index_build / cpd_conv_outset index against the site list, every word"""
        occ = (R.lookup(idx, self.batch, self.shape).reshape(-1) >= 0)
        bits = np.zeros(self.words * 64, bool)
        bits[:self.cells] = occ
        want_words = np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)
        np.testing.assert_array_equal(self.part(self.o_bitmap, self.words, np.uint64), want_words)
        cnt = bits.reshape(-1, 64).sum(1)
        np.testing.assert_array_equal(self.part(self.o_base, self.words, np.uint32), np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint32))
        blk = np.add.reduceat(cnt, np.arange(0, self.words, SCAN_TILE))
        np.testing.assert_array_equal(self.part(self.o_bsum, self.nb, np.uint32), np.concatenate([[0], np.cumsum(blk)[:-1]]).astype(np.uint32))
        if n_perm is not None:                                       # perm[rank] = position in the list, for the in-grid rows
            q = np.asarray(idx, np.int64).reshape(-1, 4)
            rows = np.flatnonzero(R.valid_rows(q, self.batch, self.shape))
            key = ((q[rows, 0] * self.shape[0] + q[rows, 1]) * self.shape[1] + q[rows, 2]) * self.shape[2] + q[rows, 3]
            perm = self.part(self.o_perm, max(self.cap, 1), np.int32)
            np.testing.assert_array_equal(perm[:rows.size], rows[np.argsort(key)])
            assert (perm[rows.size:].view(np.uint8) == POISON).all()
        assert self.guard_ok()


MODES = ("canonical", "own", "installed")


def make_index(sites, batch, shape, mode, seed=0):
    """(Index, list, lookup array) of a site set in one of the three order modes: `canonical` -- the canonical list, row = rank
    (flags 0); `own` -- a shuffled list, row = its position, through the index's own map (flags 1); `installed` -- row =
    map[rank] for a caller-installed map (flags 2: cpd_index_set_order)."""
    sites = R.canonical(sites, batch, shape)
    n = sites.shape[0]
    ix = Index(batch, shape, n)
    if mode == "own":
        lst = R.shuffled(sites, seed + 1)
        assert ix.build(lst) == OK
        return ix, lst, R.lookup(lst, batch, shape)
    assert ix.build(sites) == OK
    if mode == "canonical":
        ix.set_order(None)
        return ix, sites, R.lookup(sites, batch, shape, np.arange(n))
    rmap = np.random.default_rng(seed + 2).permutation(n).astype(np.int32)
    ix.set_order(rmap)
    return ix, sites, R.lookup(sites, batch, shape, rmap)


def table(ix, out_idx, ksize, stride=None, pad=None, mask=True):
    """cpd_rulebook_subm (stride None) / cpd_rulebook_conv over `out_idx` -> (rc, nbr [kv, n] or the raw fenced tensor on error, mask)"""
    out_idx = np.asarray(out_idx, np.int32).reshape(-1, 4)
    n, kv = out_idx.shape[0], ksize[0] * ksize[1] * ksize[2]
    d_out, nbr, tm = dev(out_idx), fenced(kv * n), fenced((n + 15) // 16) if mask else None
    if stride is None:
        rc = L().cpd_rulebook_subm(_lib.ptr(d_out), n, ix.batch, _lib.iarr(ix.shape), _lib.iarr(ksize), ix.ptr(), _lib.ptr(nbr), _lib.ptr(tm), _lib.stream())
    else:
        rc = L().cpd_rulebook_conv(_lib.ptr(d_out), n, ix.batch, _lib.iarr(ix.shape), _lib.iarr(ksize), _lib.iarr(stride), _lib.iarr(pad), ix.ptr(),
                                   _lib.ptr(nbr), _lib.ptr(tm), _lib.stream())
    if rc != OK:
        return rc, nbr, tm
    return rc, host(nbr, kv * n, (kv, n)), (host(tm, dtype=np.uint32) if mask else None)


def emit(ix, cap):
    out = fenced(4 * cap)
    assert L().cpd_index_emit(ix.ptr(), ix.batch, _lib.iarr(ix.shape), _lib.ptr(out), cap, _lib.stream()) == OK
    return host(out, 4 * cap, (cap, 4))


def check_table(ix, lut, out_idx, ksize, stride=None, pad=None):
    kv = ksize[0] * ksize[1] * ksize[2]
    rc, nbr, tm = table(ix, out_idx, ksize, stride, pad, mask=True)
    assert rc == OK
    want = R.subm_table(lut, out_idx, ksize) if stride is None else R.conv_table(lut, out_idx, ksize, stride, pad)
    np.testing.assert_array_equal(nbr, want)
    if kv <= 32:
        np.testing.assert_array_equal(tm, R.tapmask(want))
    else:
        assert (tm == PATTERN).all()                                 # no tap masks beyond 32 taps: the words stay as they were


# =================================================================================================== A. bitmap word geometry
A_KSIZES = [[3, 3, 3], [1, 1, 1], [3, 1, 1], [1, 3, 3], [5, 5, 1], [3, 3, 5], [1, 1, 31]]
A_WIDTHS = [1, 2, 3, 31, 63, 64, 65, 127, 129]


def _geometry(batch, shape):
    for name, g in R.GENERATORS.items():
        sites = g(batch, shape)
        for order in ("canonical", "shuffled"):
            lst = sites if order == "canonical" else R.shuffled(sites, 5)
            ix = Index(batch, shape, len(lst))
            assert ix.build(lst) == OK, (name, order)
            ix.check(lst, n_perm=len(lst))
            lut = R.lookup(lst, batch, shape)
            for k in A_KSIZES:
                check_table(ix, lut, lst, k)
            np.testing.assert_array_equal(emit(ix, len(sites)), sites, err_msg="%s %s" % (name, order))


@gpu
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("W", A_WIDTHS)
def test_a_rows_start_at_every_bit_offset(hip, W, batch):
    """x-lines of W cells in grids of D, H in {1, 2, 5}: with W odd the lines start at every bit offset of a word, a 3-, 5- or
    31-cell tap run crosses words, and the last word is partial"""
    for D in (1, 2, 5):
        for H in (1, 2, 5):
            _geometry(batch, [D, H, W])


@gpu
@pytest.mark.parametrize("cells", [1, 63, 64, 65, 128])
def test_a_one_or_two_words(hip, cells):
    _geometry(1, [1, 1, cells])


@gpu
def test_a_refused_kernels_write_nothing(hip):
    batch, shape = 1, [2, 3, 70]
    sites = R.gen_random(0.5)(batch, shape)
    ix, lst, _ = make_index(sites, batch, shape, "own")
    for k, want in [([1, 1, 33], UNSUPPORTED), ([3, 3, 2], ARG), ([2, 1, 1], ARG), ([1, 4, 1], ARG), ([0, 1, 1], ARG)]:
        rc, nbr, tm = table(ix, lst, k)
        assert rc == want, k
        assert untouched(nbr) and untouched(tm)
    rc, nbr, tm = table(ix, lst[:5], [1, 1, 33], ONE, [0, 0, 16])    # the strided builder has the same two-word limit
    assert rc == UNSUPPORTED and untouched(nbr) and untouched(tm)


# =================================================================================================== B. scan edges
def _scan_case(words, site_words):
    """grid [1, words, 64]: x-line y IS bitmap word y. Sites at bits 0, 5 and 63 of the given words; ranks through the centre tap
    of a (1, 1, 1) table on the canonical index (row = rank), through cpd_index_emit, and the prefix words themselves."""
    shape = [1, words, 64]
    sites = np.array([[0, 0, w, x] for w in site_words for x in (0, 5, 63)], np.int32)
    n = len(sites)
    ix = Index(1, shape, n)
    assert ix.build(sites) == OK
    ix.set_order(None)
    rc, nbr, _ = table(ix, sites, ONE, mask=False)
    assert rc == OK
    np.testing.assert_array_equal(nbr[0], np.arange(n))
    np.testing.assert_array_equal(emit(ix, n), sites)
    # the prefix at every site word and at its neighbours (empty words of blocks the full scan still covers)
    for w in site_words:
        for ww in (w - 1, w, w + 1):
            if 0 <= ww < words:
                assert int(ix.part(ix.o_base + 4 * ww, 1, np.uint32)[0]) == 3 * sum(1 for v in site_words if v < ww), (w, ww)
        assert int(ix.part(ix.o_bitmap + 8 * w, 1, np.uint64)[0]) == (1 | 1 << 5 | 1 << 63)
    blocks = (words + SCAN_TILE - 1) // SCAN_TILE
    want_bsum = [3 * sum(1 for w in site_words if w // SCAN_TILE < b) for b in range(blocks)]
    np.testing.assert_array_equal(ix.part(ix.o_bsum, blocks, np.uint32), np.array(want_bsum, np.uint32))
    assert ix.guard_ok()
    return ix


@gpu
@pytest.mark.parametrize("words", [4095, 4096, 4097, 8193])
def test_b_scan_tile_edges(hip, words):
    blocks = (words + SCAN_TILE - 1) // SCAN_TILE
    ends = sorted({w for b in range(blocks) for w in (b * SCAN_TILE, min(words, (b + 1) * SCAN_TILE) - 1)})
    ix = _scan_case(words, ends)                                     # the first and the last word of every scan block
    ix.check(np.array([[0, 0, w, x] for w in ends for x in (0, 5, 63)], np.int32))
    _scan_case(words, [words - 1])                                   # everything in the last word


@gpu
def test_b_spine_second_trip(hip):
    """1025 scan blocks (2.7e8 cells, 50 MB of index): the spine's 1024 threads take a second trip; sites in blocks 0, 1023, 1024"""
    words = 1024 * SCAN_TILE + 1
    _scan_case(words, [7, 1023 * SCAN_TILE + 9, 1024 * SCAN_TILE - 1, 1024 * SCAN_TILE])


# =================================================================================================== C. row counts of the row-per-lane rulebook
C_ROWS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513]
C_SHAPE = [7, 10, 18]                # box: 5 x 8 x 16 = 640 rows
C_IN = [13, 19, 35]                  # the input grid whose stride-2 output grid is C_SHAPE


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", C_ROWS)
def test_c_subm_row_counts(hip, n, mode):
    sites = R.gen_box(1, C_SHAPE)[:n]
    ix, lst, lut = make_index(sites, 1, C_SHAPE, mode, seed=n)
    check_table(ix, lut, lst, [3, 3, 3])                             # K3 instantiation, 27 mask bits
    check_table(ix, lut, lst, [1, 3, 5])                             # runtime extents, 15 mask bits
    check_table(ix, lut, lst, [3, 3, 5])                             # 45 taps: the mask words stay untouched ...
    rc, nbr, _ = table(ix, lst, [3, 3, 5], mask=False)               # ... and a NULL mask is fine
    assert rc == OK
    np.testing.assert_array_equal(nbr, R.subm_table(lut, lst, [3, 3, 5]))
    if mode == "installed":                                          # back to canonical: row = rank again
        ix.set_order(None)
        check_table(ix, R.lookup(lst, 1, C_SHAPE, np.arange(len(lst))), lst, [3, 3, 3])
    assert ix.guard_ok()


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", C_ROWS)
def test_c_strided_row_counts(hip, n, mode):
    sites = R.gen_random(0.5)(1, C_IN)
    ix, lst, lut = make_index(sites, 1, C_IN, mode, seed=n)
    outs = R.gen_box(1, C_SHAPE)[:n]
    assert R.out_shape(C_IN, [3, 3, 3], [2, 2, 2], ONE) == C_SHAPE
    check_table(ix, lut, outs, [3, 3, 3], [2, 2, 2], ONE)
    check_table(ix, lut, outs, [1, 3, 5], [2, 2, 2], [0, 1, 2])
    check_table(ix, lut, outs, [3, 3, 5], [2, 2, 2], [1, 1, 2])
    rc, nbr, _ = table(ix, outs, [3, 3, 5], [2, 2, 2], [1, 1, 2], mask=False)
    assert rc == OK
    np.testing.assert_array_equal(nbr, R.conv_table(lut, outs, [3, 3, 5], [2, 2, 2], [1, 1, 2]))
    if mode == "installed":
        ix.set_order(None)
        check_table(ix, R.lookup(lst, 1, C_IN, np.arange(len(lst))), outs, [3, 3, 3], [2, 2, 2], ONE)
    assert ix.guard_ok()


# =================================================================================================== D. strided output sets and tables
D_CONVS = {"k3s2p1": ([3, 3, 3], [2, 2, 2], [1, 1, 1]), "k3s2p011": ([3, 3, 3], [2, 2, 2], [0, 1, 1]), "k311s211": ([3, 1, 1], [2, 1, 1], [0, 0, 0]),
           "k3s1p0": ([3, 3, 3], ONE, [0, 0, 0]), "k2s2p0": ([2, 2, 2], [2, 2, 2], [0, 0, 0]), "k3s3p1": ([3, 3, 3], [3, 3, 3], ONE),
           "k5s3p2": ([5, 5, 5], [3, 3, 3], [2, 2, 2]), "k7s3p3": ([7, 7, 7], [3, 3, 3], [3, 3, 3]),
           "k1x1x32": ([1, 1, 32], ONE, [0, 0, 16]), "k3x1x5": ([3, 1, 5], [2, 1, 3], [0, 0, 2])}
D_GENS = ["lines", "full", "word_edges", "random50"]


def outset_dev(lst, batch, in_shape, k, s, p):
    """cpd_conv_outset into a poisoned index -> (Index over the output grid, n_out)"""
    oshape = R.out_shape(in_shape, k, s, p)
    ox = Index(batch, oshape, 0)
    d_in, cnt = dev(lst.reshape(-1, 4)), fenced(1)
    rc = L().cpd_conv_outset(_lib.ptr(d_in), d_in.shape[0], batch, _lib.iarr(in_shape), _lib.iarr(k), _lib.iarr(s), _lib.iarr(p), ox.ptr(), ox.bytes,
                             _lib.ptr(cnt), _lib.stream())
    assert rc == OK
    return ox, int(host(cnt, 1)[0])


@gpu
@pytest.mark.parametrize("wo", [63, 64, 65, 130])
@pytest.mark.parametrize("conv", list(D_CONVS))
def test_d_output_sets(hip, conv, wo):
    k, s, p = D_CONVS[conv]
    batch = 2
    in_shape = [2 * s[0] + k[0] - 2 * p[0], s[1] + k[1] - 2 * p[1], (wo - 1) * s[2] + k[2] - 2 * p[2]]      # the smallest grid with 3 x 2 x wo outputs
    assert R.out_shape(in_shape, k, s, p) == [3, 2, wo]
    for gname in D_GENS:
        full = R.GENERATORS[gname](batch, in_shape)
        if gname == "random50":
            full = R.shuffled(full, 3)
        for n_in in (len(full), 1, 63, 64, 65, 257):
            if n_in > len(full):
                continue
            lst = full[len(full) - n_in:] if gname != "random50" else full[:n_in]     # (the tail keeps the last cell of the grid in)
            want = R.outset(lst, batch, in_shape, k, s, p)
            ox, n_out = outset_dev(lst, batch, in_shape, k, s, p)
            assert n_out == len(want), (gname, n_in)
            ox.check(want)                                           # every bitmap and prefix word of the output index
            np.testing.assert_array_equal(emit(ox, n_out), want, err_msg="%s %d" % (gname, n_in))
            cap = n_out // 2                                         # a capacity below the count: exactly `cap` rows are written
            np.testing.assert_array_equal(emit(ox, cap), want[:cap])
            ix = Index(batch, in_shape, len(lst))
            assert ix.build(lst) == OK
            check_table(ix, R.lookup(lst, batch, in_shape), want, k, s, p)


# =================================================================================================== E. tap-pattern order
E_SHAPE = [24, 42, 42]               # box: 22 x 40 x 40 = 35200 rows, its interior reaches into any ragged last chunk
CHUNKS = [1024, 4096, 8192, 16384]


def order_by_taps(ix, lst, n, ksize, chunk, with_coords=True):
    """cpd_order_rows_by_taps over the first n rows of `lst` -> (rc, new_to_old, old_to_new, coords) fenced tensors"""
    d_in = dev(lst[:n].reshape(-1, 4))
    n2o, o2n, out = fenced(n), fenced(n), fenced(4 * n) if with_coords else None
    ws = poison(max(n, 1) * 4)
    rc = L().cpd_order_rows_by_taps(_lib.ptr(d_in), n, ix.batch, _lib.iarr(ix.shape), _lib.iarr(ksize), ix.ptr(), chunk, _lib.ptr(n2o), _lib.ptr(o2n),
                                    _lib.ptr(out), _lib.ptr(ws), max(n, 1) * 4, _lib.stream())
    assert (ws[max(n, 1) * 4:] == POISON).all().item()
    return rc, n2o, o2n, out


def check_tap_order(ix, lut, lst, n, ksize, chunk):
    """the index may hold more sites than the n rows being ordered: their patterns see all of them"""
    rc, n2o, o2n, out = order_by_taps(ix, lst, n, ksize, chunk)
    assert rc == OK
    pat = R.row_pattern(R.subm_table(lut, lst[:n], ksize))
    w_n2o, w_o2n = R.tap_order(pat, chunk)
    np.testing.assert_array_equal(host(n2o, n), w_n2o)
    np.testing.assert_array_equal(host(o2n, n), w_o2n)
    np.testing.assert_array_equal(host(out, 4 * n, (n, 4)), lst[:n][w_n2o])
    return pat, w_n2o


@pytest.fixture(scope="module")
def e_box():
    """the box's rows starting in the middle of its fifth z-layer: every prefix of the list, and the ragged last chunk of every row
    count used below, has interior rows (all 27 neighbours: the padding rows' key) next to face and edge rows"""
    box = R.gen_box(1, E_SHAPE)
    sites = np.concatenate([box[8000:], box[:8000]])
    return sites, R.lookup(sites, 1, E_SHAPE)


@gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_e_ragged_chunks_tie_with_the_padding_key(hip, e_box, chunk):
    sites, lut = e_box
    ix = Index(1, E_SHAPE, len(sites))
    assert ix.build(sites) == OK
    for n in (1, chunk - 1, chunk, chunk + 1, 2 * chunk + 17):
        pat, n2o = check_tap_order(ix, lut, sites, n, [3, 3, 3], chunk)
        if n in (chunk - 1, 2 * chunk + 17):                         # real rows with the padding rows' key sit in the ragged chunk
            assert (pat[n - n % chunk:] == R.PAD_KEY).any()
    assert (pat != R.PAD_KEY).any()
    assert ix.guard_ok()


@gpu
def test_e_equal_patterns_keep_their_order(hip):
    batch, shape = 2, [9, 30, 30]
    q = R.gen_full(batch, shape)
    sites = q[(q[:, 1] % 2 == 0) & (q[:, 2] % 2 == 0) & (q[:, 3] % 2 == 0)]      # isolated: only the centre tap everywhere
    ix, lst, lut = make_index(sites, batch, shape, "canonical")
    for chunk in CHUNKS:
        pat, n2o = check_tap_order(ix, lut, lst, len(lst), [3, 3, 3], chunk)
        assert (pat == 1 << 13).all() and (n2o == np.arange(len(lst))).all()


@gpu
@pytest.mark.parametrize("digit", [0, 1, 2, 3])
def test_e_each_radix_pass_decides(hip, digit):
    """Centre sites on a lattice of pitch 3, each with its own subset of neighbours drawn from the taps of ONE 7-bit digit of the
    key (thin slabs, rods and pairs along z, y and x); only the centres are ordered, the neighbours are in the index alone. The
    patterns then differ in that digit only, so that radix pass alone decides the order."""
    taps = [t for t in range(7 * digit, min(27, 7 * digit + 7)) if t != 13]
    shape = [51, 48, 48]
    a = np.stack(np.meshgrid(np.arange(17), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3) * 3 + 1
    rng = np.random.default_rng(digit)
    centres = np.concatenate([np.zeros((len(a), 1), np.int64), a], 1)
    extra = []
    for i, c in enumerate(centres):
        sub = rng.integers(0, 1 << len(taps)) if i % 5 else (1 << (i // 5 % len(taps)))     # every fifth: a pair (one neighbour)
        for bit, t in enumerate(taps):
            if sub >> bit & 1:
                extra.append(c + [0, t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1])
    lst = np.concatenate([centres, np.array(extra, np.int64)]).astype(np.int32)
    ix = Index(1, shape, len(lst))
    assert ix.build(lst) == OK
    lut = R.lookup(lst, 1, shape)
    for chunk, n in ((1024, 1041), (4096, 4113), (8192, len(centres))):
        pat, _ = check_tap_order(ix, lut, lst, n, [3, 3, 3], chunk)
        varying = int(np.bitwise_or.reduce(pat ^ pat[0]))
        lo, hi = 7 * digit, min(27, 7 * digit + 7)
        assert varying and varying >> hi == 0 and varying & ((1 << lo) - 1) == 0, hex(varying)
        assert len(np.unique(pat)) > 16


@gpu
@pytest.mark.parametrize("ksize", [[3, 3, 1], [3, 1, 1]])
def test_e_other_kernels(hip, ksize):
    batch, shape = 2, [6, 20, 33]
    for gname in ("box", "random50", "checker"):
        ix, lst, lut = make_index(R.GENERATORS[gname](batch, shape), batch, shape, "own")
        for chunk in (1024, 4096):
            check_tap_order(ix, lut, lst, len(lst), ksize, chunk)


@gpu
def test_e_refusals_write_nothing(hip, e_box):
    sites, _ = e_box
    ix = Index(1, E_SHAPE, len(sites))
    assert ix.build(sites) == OK
    for ksize, chunk, want in [([3, 3, 3], 2048, UNSUPPORTED), ([3, 3, 5], 4096, UNSUPPORTED), ([1, 1, 33], 4096, UNSUPPORTED), ([3, 3, 2], 4096, ARG)]:
        rc, n2o, o2n, out = order_by_taps(ix, sites, 100, ksize, chunk)
        assert rc == want, (ksize, chunk)
        assert untouched(n2o) and untouched(o2n) and untouched(out)


# =================================================================================================== F. chunk-ordered rulebook
F_ROWS = [1, 15, 1023, 1024, 1025, 4095, 4096, 4097, 8192 + 17]
F_IN = [13, 80, 80]                  # stride 2: 7 x 40 x 40 (pad 1) or 6 x 40 x 40 (pad 0 in z) output cells, nearly all active
F_CONVS = {"s1": (ONE, ONE), "s2p111": ([2, 2, 2], ONE), "s2p011": ([2, 2, 2], [0, 1, 1])}


def chunk_ordered(ix, out_canon, o2n, stride, pad, ksize=(3, 3, 3), chunk=4096):
    n = len(out_canon)
    d_out, d_o2n = dev(out_canon.reshape(-1, 4)), None if o2n is None else dev(o2n)
    nbr, tm = fenced(27 * n), fenced((n + 15) // 16)
    rc = L().cpd_rulebook_chunk_ordered(_lib.ptr(d_out), _lib.ptr(d_o2n), n, ix.batch, _lib.iarr(ix.shape), _lib.iarr(ksize), _lib.iarr(stride),
                                        _lib.iarr(pad), ix.ptr(), chunk, _lib.ptr(nbr), _lib.ptr(tm), _lib.stream())
    return rc, nbr, tm


@pytest.fixture(scope="module")
def f_sites():
    return {"s1": R.gen_box(1, E_SHAPE), "s2": R.gen_random(0.5)(1, F_IN)}


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("conv", list(F_CONVS))
def test_f_chunk_ordered_tables(hip, f_sites, conv, mode):
    stride, pad = F_CONVS[conv]
    in_shape = E_SHAPE if conv == "s1" else F_IN
    sites = f_sites["s1" if conv == "s1" else "s2"]
    ix, lst, lut = make_index(sites, 1, in_shape, mode)
    level = R.canonical(sites, 1, in_shape) if conv == "s1" else R.outset(sites, 1, in_shape, [3, 3, 3], stride, pad)
    oshape = R.out_shape(in_shape, [3, 3, 3], stride, pad)
    assert len(level) >= F_ROWS[-1]
    for n in F_ROWS:
        out = level[:n]
        # the order from E: the out level's own index, its rows sorted by sub-manifold pattern inside chunks of 4096
        ox = Index(1, oshape, n)
        assert ox.build(out) == OK
        rc, _, o2n_d, _ = order_by_taps(ox, out, n, [3, 3, 3], 4096, with_coords=False)
        assert rc == OK
        o2n = host(o2n_d, n)
        n2o = np.empty(n, np.int64)
        n2o[o2n] = np.arange(n)
        assert sorted(o2n) == list(range(n)) and (o2n // 4096 == np.arange(n) // 4096).all()
        for order, rows in ((None, out), (o2n, out[n2o])):
            rc, nbr, tm = chunk_ordered(ix, out, order, stride, pad)
            assert rc == OK
            want = R.conv_table(lut, rows, [3, 3, 3], stride, pad)
            np.testing.assert_array_equal(host(nbr, 27 * n, (27, n)), want, err_msg="n %d order %s" % (n, order is not None))
            np.testing.assert_array_equal(host(tm, dtype=np.uint32), R.tapmask(want))
            rc, ref_nbr, ref_tm = table(ix, rows, [3, 3, 3], stride, pad)                  # and the other device builder agrees
            assert rc == OK and (ref_nbr == want).all() and (ref_tm == R.tapmask(want)).all()
    assert ix.guard_ok()


@gpu
def test_f_refusals_write_nothing(hip, f_sites):
    ix, lst, _ = make_index(f_sites["s1"][:500], 1, E_SHAPE, "canonical")
    for ksize, chunk in [([3, 3, 1], 4096), ([1, 1, 1], 4096), ([5, 3, 3], 4096), ([3, 3, 3], 1024), ([3, 3, 3], 8192)]:
        rc, nbr, tm = chunk_ordered(ix, lst, None, ONE, ONE, ksize, chunk)
        assert rc == UNSUPPORTED, (ksize, chunk)
        assert untouched(nbr) and untouched(tm)


# =================================================================================================== G. brick order
BRICKS = [(8, 8), (4, 16), (1, 1), (64, 64)]


def order_bricks(ix, lst, by, bx, tile):
    n = len(lst)
    d_in = dev(lst.reshape(-1, 4))
    n2o, o2n, out = fenced(n), fenced(n), fenced(4 * n)
    n1 = max(n, 1)
    wsb = 2 * a256(4 * n1) + a256(16 * n1)
    ws = poison(wsb)
    rc = L().cpd_order_rows_bricks(_lib.ptr(d_in), n, ix.batch, _lib.iarr(ix.shape), ix.ptr(), by, bx, tile, _lib.ptr(n2o), _lib.ptr(o2n), _lib.ptr(out),
                                   _lib.ptr(ws), wsb, _lib.stream())
    assert (ws[wsb:] == POISON).all().item()
    return rc, n2o, o2n, out


def check_bricks(ix, lst, by, bx, tile, what=""):
    n = len(lst)
    rc, n2o, o2n, out = order_bricks(ix, lst, by, bx, tile)
    assert rc == OK
    w_out, w_n2o, w_o2n = R.brick_tile_order(lst, ix.batch, ix.shape, by, bx, tile)
    np.testing.assert_array_equal(host(n2o, n), w_n2o, err_msg=what)
    np.testing.assert_array_equal(host(o2n, n), w_o2n, err_msg=what)
    np.testing.assert_array_equal(host(out, 4 * n, (n, 4)), w_out, err_msg=what)
    return w_n2o


@gpu
@pytest.mark.parametrize("W", [7, 8, 9, 20])
@pytest.mark.parametrize("H", [7, 8, 9, 20])
def test_g_bricks_clipped_by_the_grid(hip, H, W):
    """bricks that the grid clips in y, in x and in both, sites in the last y-band of the last z-plane of the last batch (the rank
    query past the last cell), a cell count that is a multiple of 64 (H = W = 8) and ones that are not"""
    batch, shape = 2, [2, H, W]
    for gname in ("full", "random50", "box", "lines"):
        sites = R.GENERATORS[gname](batch, shape)
        for n in (len(sites), 1, 127, 128, 129, 257):
            if n > len(sites):
                continue
            for lst in (sites[len(sites) - n:], sites[:n]):          # the tail keeps the grid's last rows in, the head its first
                ix = Index(batch, shape, n)
                assert ix.build(lst) == OK
                ix.set_order(None)
                for by, bx in BRICKS:
                    for tile in (128, 256):
                        n2o = check_bricks(ix, lst, by, bx, tile, "%s n %d brick %dx%d tile %d" % (gname, n, by, bx, tile))
                        if (by, bx) == (64, 64):                     # one brick per plane: canonical up to the tile sort
                            assert (n2o // tile == np.arange(n) // tile).all()
                assert ix.guard_ok()


@gpu
def test_g_refusals(hip):
    ix, lst, _ = make_index(R.gen_full(1, [2, 8, 8]), 1, [2, 8, 8], "canonical")
    for by, bx, tile, want in [(8, 8, 64, UNSUPPORTED), (8, 8, 512, UNSUPPORTED), (0, 8, 128, ARG), (8, -1, 128, ARG)]:
        rc, n2o, o2n, out = order_bricks(ix, lst, by, bx, tile)
        assert rc == want and untouched(n2o) and untouched(o2n) and untouched(out)


@gpu
@pytest.mark.parametrize("n", [1, 65])
def test_g_row_orders_refuse_a_short_workspace(hip, n):
    """Both row orders check their workspace against their own size query: a view 256 bytes shorter than the query's answer (for
    cpd_order_rows_by_taps, whose answer is 4 n bytes and not rounded up, as many bytes shorter as there are) is refused with
    CPD_ERR_WORKSPACE and nothing is written. The view is the head of a buffer of the full size, so a check that wrongly let the
    call through would still write inside the allocation."""
    shape = [2, 8, 8]
    ix, lst, _ = make_index(R.gen_full(1, shape)[:n], 1, shape, "canonical")
    assert len(lst) == n
    d_in = dev(lst.reshape(-1, 4))
    for name in ("bricks", "by_taps"):
        need = getattr(L(), "cpd_order_rows_%s_workspace_bytes" % name)(n)
        full = poison(need)
        view = full[:max(need - 256, 0)]                             # same base address as `full`
        assert view.numel() < need
        n2o, o2n, out = fenced(n), fenced(n), fenced(4 * n)
        tail = (_lib.ptr(n2o), _lib.ptr(o2n), _lib.ptr(out), _lib.ptr(full), view.numel(), _lib.stream())
        if name == "bricks":
            rc = L().cpd_order_rows_bricks(_lib.ptr(d_in), n, ix.batch, _lib.iarr(ix.shape), ix.ptr(), 8, 8, 128, *tail)
        else:
            rc = L().cpd_order_rows_by_taps(_lib.ptr(d_in), n, ix.batch, _lib.iarr(ix.shape), _lib.iarr([3, 3, 3]), ix.ptr(), 4096, *tail)
        assert rc == WORKSPACE, name
        assert untouched(n2o) and untouched(o2n) and untouched(out) and bool((full == POISON).all().item()), name
    assert ix.guard_ok()


V_SHAPE = [5, 600, 500]              # the index's grid: the voxel grid 4 x 600 x 500 and one more z-level (the backbone's sparse shape)
V_VSIZE, V_RANGE = [1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 500.0, 600.0, 4.0]
V_BLOCK = 64 * SCAN_TILE             # cells per scan block: 524.288 x-lines of 500 cells -- block edges fall inside lines, bands and bricks
V_EDGES = (1, 4, 6, 9)               # the scan-block edges a patch of voxels sits right behind


def _voxel_cloud():
    """Two frames of points whose voxels sit right BEHIND a few scan-block edges, the block in front of each edge without a
    single site: a patch of ten x-lines starting with the line after the one the edge cuts, 60 cells wide around the edge's x. The
    rows of such a patch share y-bands and bricks with cells in front of the edge, so the brick order's rank queries -- the start
    of the band, the brick's left and right edge in the earlier lines -- land in words of a block that holds no site.
    -> (canonical voxel coordinates, the frames' points)"""
    rng = np.random.default_rng(12)
    D, H, W = V_SHAPE
    cells = []
    for e in V_EDGES:
        line, x_cut = divmod(e * V_BLOCK, W)
        f, z, y = line // (D * H), line // H % D, line % H
        assert f < 2 and z < D - 1 and y % 64 < 50 and 30 <= x_cut < W - 30      # the patch stays in its plane and in the edge line's 64-line band
        yy, xx = np.meshgrid(np.arange(y + 1, y + 11), np.arange(x_cut - 30, x_cut + 30), indexing="ij")
        keep = rng.random(yy.shape) < 0.7
        cells += [(f, z, int(a), int(b)) for a, b in zip(yy[keep], xx[keep])]
    cells = np.unique(np.array(cells, np.int64), axis=0)
    reps = rng.integers(1, 4, len(cells))
    rows = np.repeat(cells, reps, axis=0)[rng.permutation(int(reps.sum()))]
    pts = np.empty((len(rows), 4), np.float32)
    pts[:, 0] = rows[:, 3] + rng.uniform(0.1, 0.9, len(rows))
    pts[:, 1] = rows[:, 2] + rng.uniform(0.1, 0.9, len(rows))
    pts[:, 2] = rows[:, 1] + rng.uniform(0.1, 0.9, len(rows))
    pts[:, 3] = rng.random(len(rows))
    return cells.astype(np.int32), [pts[rows[:, 0] == f] for f in (0, 1)]


@gpu
def test_g_index_left_by_the_batched_voxelizer(hip):
    """The contract of site_index_layout.h: an index built by cpd_voxelize_batch_canonical has prefix words only for the scan blocks
    that hold a site -- the others keep whatever the buffer held (here: the poison) -- and a rank query (index_rank_before) must
    answer from the block sums there. cpd_order_rows_bricks over it equals the result over the cpd_index_build index of the same
    coordinates, and both equal the restatement."""
    cells, frames = _voxel_cloud()
    nf, c, P = 2, 4, 5
    shape = V_SHAPE
    offs = [0, len(frames[0]), len(frames[0]) + len(frames[1])]
    n_pts = offs[-1]
    pts = dev(np.concatenate(frames), np.float32)
    vs, rg = _lib.farr(V_VSIZE), _lib.farr(V_RANGE)
    ix = Index(nf, shape, n_pts)
    wsb = L().cpd_voxelize_batch_workspace_bytes(n_pts, nf, P, n_pts, vs, rg)
    assert wsb > 0
    ws = poison(wsb)
    coords, num, mean, nvox = fenced(4 * n_pts), fenced(n_pts), torch.empty((n_pts, c), device="cuda"), fenced(nf + 1)
    rc = L().cpd_voxelize_batch_canonical(_lib.ptr(pts), _lib.iarr(offs), nf, c, vs, rg, P, n_pts, None, _lib.ptr(coords), _lib.ptr(num), _lib.ptr(mean),
                                          _lib.ptr(nvox), _lib.ptr(ws), wsb, ix.ptr(), ix.bytes, 1, _lib.stream())
    assert rc == OK
    n = len(cells)
    nv = host(nvox, nf + 1)
    assert list(nv) == [int((cells[:, 0] == 0).sum()), int((cells[:, 0] == 1).sum()), n]
    got = host(coords, 4 * n_pts).reshape(-1, 4)[:n]
    np.testing.assert_array_equal(got, cells)                        # canonical rows
    # what the voxelizer left behind: the bitmap complete, the block sums complete, prefix words ONLY in blocks with a site
    occ = np.zeros(ix.words * 64, bool)
    key = ((cells[:, 0].astype(np.int64) * shape[0] + cells[:, 1]) * shape[1] + cells[:, 2]) * shape[2] + cells[:, 3]
    occ[key] = True
    cnt = occ.reshape(-1, 64).sum(1)
    np.testing.assert_array_equal(ix.part(ix.o_bitmap, ix.words, np.uint64), np.packbits(occ.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))
    blk = np.add.reduceat(cnt, np.arange(0, ix.words, SCAN_TILE))
    assert list(np.flatnonzero(blk)) == list(V_EDGES) and ix.nb == 12
    # the queries this test is about: band starts and brick edges of occupied rows that lie in a block without a site
    for by, bx in ((8, 8), (64, 64)):
        band0 = key - (cells[:, 2] % by) * shape[2] - cells[:, 3]
        left = key - (cells[:, 2] % by) * shape[2] - cells[:, 3] % bx
        assert (blk[band0 // V_BLOCK] == 0).any() and (blk[left // V_BLOCK] == 0).any()
    np.testing.assert_array_equal(ix.part(ix.o_bsum, ix.nb + 1, np.uint32), np.concatenate([[0], np.cumsum(blk)]).astype(np.uint32))
    base = ix.part(ix.o_base, ix.words, np.uint32)
    want_base = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint32)
    covered = blk[np.arange(ix.words) // SCAN_TILE] > 0              # per word: does its scan block hold a site
    np.testing.assert_array_equal(base[covered], want_base[covered])
    assert (base[~covered].view(np.uint8) == POISON).all()           # the partial prefix this test is about
    assert ix.part(0, 1, np.int32)[0] == 0 and ix.guard_ok()         # flags: canonical
    # lookups test the bit first: the tables are complete
    lut = R.lookup(cells, nf, shape, np.arange(n))
    check_table(ix, lut, cells, [3, 3, 3])
    np.testing.assert_array_equal(emit(ix, n), cells)
    ref = Index(nf, shape, n)
    assert ref.build(cells) == OK
    ref.set_order(None)
    for by, bx in BRICKS:
        for tile in (128, 256):
            rc, n2o, o2n, out = order_bricks(ix, cells, by, bx, tile)
            rc2, n2o2, o2n2, out2 = order_bricks(ref, cells, by, bx, tile)
            assert rc == OK and rc2 == OK
            w_out, w_n2o, w_o2n = R.brick_tile_order(cells, nf, shape, by, bx, tile)
            for a, b, w in ((n2o, n2o2, w_n2o), (o2n, o2n2, w_o2n)):
                np.testing.assert_array_equal(host(b, n), w)
                np.testing.assert_array_equal(host(a, n), w, err_msg="voxelizer-built index, brick %dx%d tile %d" % (by, bx, tile))
            np.testing.assert_array_equal(host(out, 4 * n, (n, 4)), w_out)
            assert torch.equal(out, out2)


# =================================================================================================== H. densify
H_SPECIAL = np.array([0x80000000, 0x7fc12345, 0xffa00001, 0x00000001, 0x807fffff, 0x7f800000], np.uint32)   # -0.0, NaNs with payloads, denormals, inf


def _payload(n, c, seed):
    f = np.random.default_rng(seed).integers(1, 2 ** 32, (n, c), dtype=np.uint64).astype(np.uint32)
    flat = f.reshape(-1)
    flat[:min(flat.size, H_SPECIAL.size)] = H_SPECIAL[:flat.size]
    return f


def _corners(batch, shape):
    return np.array([[b, z, y, x] for b in (0, batch - 1) for z in {0, shape[0] - 1} for y in (0, shape[1] - 1) for x in (0, shape[2] - 1)], np.int32)


def densify_dev(name, feat, idx, c, batch, shape, out):
    d_f, d_i = dev(feat.view(np.int32)), dev(idx.reshape(-1, 4))
    n = d_i.shape[0]
    if name == "clear":
        return L().cpd_densify_nhwc_clear(_lib.ptr(d_i), n, c, batch, _lib.iarr(shape), _lib.ptr(out), _lib.stream())
    fn = getattr(L(), "cpd_densify_" + name)
    return fn(_lib.ptr(d_f), _lib.ptr(d_i), n, c, batch, _lib.iarr(shape), _lib.ptr(out), _lib.stream())


H_GRIDS = {"small": (2, [3, 4, 5]), "flat": (2, [1, 4, 5]), "big": (2, [2, 40, 52])}      # big: a map above 1 MiB at c = 64 (the fill kernel)


@gpu
@pytest.mark.parametrize("grid", list(H_GRIDS))
@pytest.mark.parametrize("c", [1, 3, 4, 5, 64])
def test_h_densify_layouts(hip, c, grid):
    batch, shape = H_GRIDS[grid]
    total = batch * shape[0] * shape[1] * shape[2] * c
    corners = np.unique(_corners(batch, shape), axis=0)
    rnd = R.gen_random(0.05 if grid == "big" else 0.3)(batch, shape)
    for what, idx in (("none", np.zeros((0, 4), np.int32)), ("corners", corners), ("mixed", R.shuffled(np.unique(np.concatenate([corners, rnd]), axis=0)))):
        f = _payload(len(idx), c, len(idx) + c)
        refs = {"nchw": R.densify_nchw(f, idx, batch, shape), "nhwc_cd": R.densify_nhwc_cd(f, idx, batch, shape)}
        if c % 4 == 0:
            refs["nhwc"] = R.densify_nhwc(f, idx, batch, shape)
        for name in ("nchw", "nhwc_cd", "nhwc"):
            out = fenced(total)
            rc = densify_dev(name, f, idx, c, batch, shape, out)
            if name not in refs:                                     # z * C + c forms move float4s: c % 4 != 0 is refused, nothing written
                assert rc == ARG and untouched(out)
                continue
            assert rc == OK
            np.testing.assert_array_equal(host(out, total, dtype=np.uint32), refs[name].reshape(-1), err_msg="%s %s" % (name, what))
        # rows into a persistent map, then clear: first a map of zeros (the contract), then a map of pattern (what else is touched?)
        for fill in (0, PATTERN):
            out = fenced(total)
            out[:total] = fill
            before = np.full(total, fill, np.uint32)
            rc = densify_dev("nhwc_rows", f, idx, c, batch, shape, out)
            if c % 4:
                assert rc == ARG and densify_dev("clear", f, idx, c, batch, shape, out) == ARG
                assert (host(out, total, dtype=np.uint32) == before).all()
                continue
            assert rc == OK
            want = R.densify_nhwc_rows(before.reshape(batch, shape[1], shape[2], shape[0] * c), f, idx, shape)
            np.testing.assert_array_equal(host(out, total, dtype=np.uint32), want.reshape(-1))
            assert densify_dev("clear", f, idx, c, batch, shape, out) == OK
            want = R.densify_nhwc_clear(want, idx, c, shape)
            got = host(out, total, dtype=np.uint32)
            np.testing.assert_array_equal(got, want.reshape(-1))
            if fill == 0:
                assert not got.any()                                 # the persistent map is all-zero again, bit for bit


@gpu
def test_h_conv2d_table(hip):
    for batch, h, w, kh, kw, s, p in [(1, 1, 1, 1, 1, 1, 0), (2, 5, 7, 3, 3, 1, 1), (1, 16, 17, 3, 3, 2, 1), (3, 9, 29, 2, 2, 2, 0), (1, 7, 5, 5, 3, 3, 2)]:
        want = R.conv2d_table(batch, h, w, kh, kw, s, p)
        nbr = fenced(want.size)
        assert L().cpd_rulebook_conv2d(batch, h, w, kh, kw, s, p, _lib.ptr(nbr), _lib.stream()) == OK
        np.testing.assert_array_equal(host(nbr, want.size, want.shape), want)


# =================================================================================================== I. index building
@gpu
def test_i_rows_outside_the_grid_are_ignored(hip):
    batch, shape = 2, [3, 4, 70]
    good = R.shuffled(R.gen_random(0.3)(batch, shape), 2)
    bad = np.array([[-1, 0, 0, 0], [batch, 0, 0, 0], [0, -1, 0, 0], [0, shape[0], 0, 0], [0, 0, -1, 0], [0, 0, shape[1], 0], [0, 0, 0, -1],
                    [0, 0, 0, shape[2]], [batch - 1, shape[0] - 1, shape[1] - 1, shape[2]], [0, 0, 1, -1]], np.int32)
    lst = np.concatenate([bad[:3], good[:11], bad[3:8], good[11:], bad[8:]])
    ix = Index(batch, shape, len(lst))
    assert ix.build(lst) == OK
    ix.check(lst, n_perm=len(lst))                                   # they shift no rank
    lut = R.lookup(lst, batch, shape)
    ok = R.valid_rows(lst, batch, shape)
    check_table(ix, lut, lst[ok], [3, 3, 3])                         # and are never returned
    np.testing.assert_array_equal(emit(ix, int(ok.sum())), R.canonical(lst, batch, shape))


@gpu
def test_i_empty_index_answers_minus_one(hip):
    batch, shape = 2, [3, 4, 70]
    ix = Index(batch, shape, 0)
    assert ix.build(np.zeros((0, 4), np.int32)) == OK
    ix.check(np.zeros((0, 4), np.int32))
    probe = R.gen_full(batch, shape)
    rc, nbr, tm = table(ix, probe, [3, 3, 3])
    assert rc == OK and (nbr == -1).all() and not tm.any()
    out = fenced(8)
    assert L().cpd_index_emit(ix.ptr(), batch, _lib.iarr(shape), _lib.ptr(out), 2, _lib.stream()) == OK
    assert untouched(out)
    ox, n_out = outset_dev(np.zeros((0, 4), np.int32), batch, shape, [3, 3, 3], [2, 2, 2], ONE)
    assert n_out == 0
    ox.check(np.zeros((0, 4), np.int32))


@gpu
def test_i_rebuilding_leaves_no_stale_bit(hip):
    batch, shape = 2, [3, 4, 70]
    big = R.gen_random(0.5)(batch, shape)
    small = R.shuffled(big[::7], 4)
    ix = Index(batch, shape, len(big))
    assert ix.build(big) == OK
    ix.check(big)
    assert ix.build(small) == OK
    ix.check(small)
    check_table(ix, R.lookup(small, batch, shape), small, [3, 3, 3])
    np.testing.assert_array_equal(emit(ix, len(small)), R.canonical(small, batch, shape))
