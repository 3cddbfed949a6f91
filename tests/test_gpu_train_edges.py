"""The kernels only the train step uses (cpd_amd/csrc/train_ops.hip) at tile, stage, block and chunk edges: the four weight-gradient
families behind T.conv_wgrad, the column reductions and row kernels of BatchNorm, and the two transposed-rulebook kernels.

The devices are those of tests/test_gpu_conv_edges.py:
  * inputs are views into wider, taller NaN-filled buffers (padding columns and the rows past n_in / n_out hold NaN): a NaN or inf
    in a result names an over-read;
  * outputs (dw, dx, dres, out, the column sums, the tables) are views into buffers that hold a fixed bit pattern: everything
    outside the view must come back bit-identical;
  * every weight-gradient launch is checked against the launch log: the instantiation the case meant is the one that ran;
  * the references are the float64 restatements of tests/ref_train_edges.py (checked on the CPU by tests/test_train_edges_ref.py).

Exact data: every entry is k / 8 with integer |k| <= 16, so every product is a multiple of 1/64 no larger than 4 and every partial
sum of up to 1536 (weight gradient) or 4097 (column sums) of them is exactly representable in fp32 -- whatever the order. Such
results are compared for EQUALITY: one missing, doubled or misplaced row changes an element by at least 1/64. Full-mantissa data
is compared under the worst-case fp32 summation bound instead, which is what sees a lost low-order term of the split arithmetic.
dy stays finite inside the region a launch owns (the fp32 kernels multiply a zero operand by the dy row where a row has no
neighbour; test_scaled_gradient_convs_do_not_hide_nan_or_overflow owns the non-finite policy).
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import ref_train_edges as R
from cpd_amd import ops, train_ops as T
from cpd_amd._lib import CpdHipError, iarr, lib, stream

gpu = pytest.mark.gpu

PATTERN = 0x5A5A5A5A                 # what every output buffer holds before a call (as a float: 1.5e16)
PITCH = {"tight": (0, 0), "wide32": (32, 32), "pad4": (4, 4), "odd": (3, 1)}      # (pitch - c, column offset of the view)
U = 2.0 ** -24                       # unit roundoff of fp32
KNOBS = ["CPD_TUNE", "CPD_WGRAD_WGS", "CPD_WGRAD_BF16X3", "CPD_COL_BLOCKS"]


def cdiv(a, b):
    return -(-a // b)


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dyadic(rng, shape):
    """k / 8, integer |k| <= 16"""
    return (rng.integers(-16, 17, size=shape) / 8.0).astype(np.float32)


def in_buffer(rows, pitch, extra=3):
    """rows [n, c] (numpy) as a device view of a NaN-filled buffer with `extra` more rows and the pitch's padding columns"""
    pad, off = PITCH[pitch]
    n, c = rows.shape
    buf = torch.full((n + extra, c + pad), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:n, off:off + c]
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows)).cuda())
    return view


def is_aligned(*views):
    """16-byte rows: what the vector forms of the kernels need of every operand"""
    return all(v is None or (v.data_ptr() % 16 == 0 and (v.dim() < 2 or v.stride(0) % 4 == 0)) for v in views)


class Flat:
    """a contiguous view of `shape` inside a flat pattern buffer, with `guard` (at least) words of pattern before and after it; the
    view starts 16-byte aligned, or 4 bytes further when `misalign` -- the way the trainer hands out views of its flat buffers"""

    def __init__(self, shape, guard, misalign=False, dtype=torch.float32):
        self.shape = tuple(shape)
        self.elems = int(np.prod(shape))
        guard = cdiv(max(guard, 4), 4) * 4
        self.off = guard + (1 if misalign else 0)
        self.flat = torch.full((self.off + self.elems + guard + 3,), PATTERN, dtype=torch.int32, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat.view(dtype)[self.off:self.off + self.elems].view(self.shape)
        assert self.view.is_contiguous() and (self.view.data_ptr() % 16 == 0) != bool(misalign)

    def check(self, label, np_dtype=np.float32):
        """-> what the view holds now; asserts that nothing outside it changed"""
        f = self.flat.cpu().numpy()
        outside = np.ones(f.shape, bool)
        outside[self.off:self.off + self.elems] = False
        stray = np.flatnonzero((f != PATTERN) & outside)
        assert stray.size == 0, (label, "wrote outside its view at words", (stray[:8] - self.off).tolist(), "view of", self.elems)
        return f.view(np_dtype)[self.off:self.off + self.elems].reshape(self.shape)

    def untouched(self):
        return bool((self.flat == PATTERN).all())


class Rows:
    """an [n, c] view of a pattern buffer with the pitch's padding columns and `guard` rows below"""

    def __init__(self, n, c, pitch, guard=4):
        pad, self.col = PITCH[pitch]
        self.n, self.c = n, c
        self.buf = torch.full((n + guard, c + pad), PATTERN, dtype=torch.int32, device="cuda")
        self.view = self.buf.view(torch.float32)[:n, self.col:self.col + c]

    def check(self, label):
        g = self.buf.cpu().numpy()
        outside = np.ones(g.shape, bool)
        outside[:self.n, self.col:self.col + self.c] = False
        stray = np.argwhere((g != PATTERN) & outside)
        assert stray.size == 0, (label, "wrote outside its rows / columns at (row, column)", stray[:8].tolist(), "n", self.n, "col", self.col)
        return np.ascontiguousarray(g.view(np.float32)[:self.n, self.col:self.col + self.c])


def exactly_representable(a64, what):
    a32 = a64.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a64), (what, "the reference itself is not an fp32 number: the premise of the exact comparison fails")
    return a32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def ulps(a, b):
    """distance of two fp32 arrays in units in the last place"""
    def key(v):
        i = bits(v).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ================================================================================================ B. weight gradient
@dataclass(frozen=True)
class Fam:
    key: str
    kind: str              # wave | tile | bf16 | f16
    c_in: int
    c_out: int
    pitches: tuple = ("tight", "tight")       # (x, dy) row pitches of a launch that does not say otherwise

    def __str__(self):
        return self.key


def _families():
    f = [Fam("wave_%d_%d" % (ci, co), "wave", ci, co) for ci in (5, 40, 72) for co in (7, 33, 65)]
    # plans as a tile launch (both channel counts multiples of 64), runs as the wave kernel: its rows are not 16-byte aligned
    f.append(Fam("wave_misaligned_64_64", "tile", 64, 64, ("odd", "tight")))
    f += [Fam("tile_%d_%d" % (ci, co), "tile", ci, co) for ci in (64, 128) for co in (64, 128)]
    for kind in ("bf16", "f16"):
        f += [Fam("%s_%d_%d" % (kind, ci, co), kind, ci, co) for ci in (32, 64, 128) for co in (32, 64, 128)]
        f += [Fam("%s_96_32" % kind, kind, 96, 32), Fam("%s_192_64" % kind, kind, 192, 64)]       # three tiles of 32 / of 64
    return f


FAMILIES = _families()
SPLIT = ("bf16", "f16")
ALL_NAMES = {"wgrad_kernel<%d,%d>" % (a, b) for a in (1, 2, 4) for b in (1, 2, 4)} | \
            {"wgrad_tile_kernel<%d,%d>" % (a, b) for a in (64, 128) for b in (64, 128)} | \
            {"wgrad_%s_kernel<%d,%d>" % (k, a, b) for k in SPLIT for a in (32, 64, 128) for b in (32, 64, 128)}
assert len(ALL_NAMES) == 9 + 4 + 9 + 9
LOGGED = set()


def lanes_per_16(c):
    return 4 if c >= 64 else (2 if c >= 32 else 1)


def split_tile(c):
    return 128 if c % 128 == 0 else (64 if c % 64 == 0 else 32)


def expected_kernel(fam, x, dy):
    """conv_wgrad_impl's selection, restated: the split kernels whenever their flag is set (both channel counts multiples of 32);
    else the tile kernel when both are multiples of 64 AND both operands have 16-byte rows; else the wave kernel"""
    if fam.kind in SPLIT:
        assert fam.c_in % 32 == 0 and fam.c_out % 32 == 0
        return "wgrad_%s_kernel<%d,%d>" % (fam.kind, split_tile(fam.c_in), split_tile(fam.c_out))
    if fam.c_in % 64 == 0 and fam.c_out % 64 == 0 and is_aligned(x, dy):
        return "wgrad_tile_kernel<%d,%d>" % (128 if fam.c_in % 128 == 0 else 64, 128 if fam.c_out % 128 == 0 else 64)
    return "wgrad_kernel<%d,%d>" % (lanes_per_16(fam.c_in), lanes_per_16(fam.c_out))


def _chunks(n_out, per_chunk, min_rows, rnd, target):
    chunks = max(1, min(cdiv(target, per_chunk), cdiv(n_out, min_rows)))
    rpc = cdiv(cdiv(n_out, chunks), rnd) * rnd
    return rpc, cdiv(n_out, rpc)


def plan(fam, n_out, kv, wgs=None):
    """(rows per chunk, chunks) of a launch: wgrad_bf16_plan / wgrad_tile_plan / wgrad_plan restated. A tile plan that falls back
    to the wave kernel keeps the tile plan's chunks."""
    ci, co = fam.c_in, fam.c_out
    if fam.kind in SPLIT:
        tm, tn = split_tile(ci), split_tile(co)
        return _chunks(n_out, kv * (ci // tm) * (co // tn), 256, 256, wgs or (512 if tm * tn >= 128 * 128 else 1024))
    if ci % 64 == 0 and co % 64 == 0:
        tm, tn = (128 if ci % 128 == 0 else 64), (128 if co % 128 == 0 else 64)
        return _chunks(n_out, kv * (ci // tm) * (co // tn), 128, 16, wgs or 512)
    per_chunk = kv * cdiv(ci, 16 * lanes_per_16(ci)) * cdiv(co, 16 * lanes_per_16(co))
    chunks = max(1, min(cdiv(8192, per_chunk), cdiv(n_out, 256), 256))
    rpc = cdiv(cdiv(n_out, chunks), 64) * 64
    return rpc, cdiv(n_out, rpc)


def chunk_rows(fam, n_out, kv, wgs=None):
    rpc, n = plan(fam, n_out, kv, wgs)
    return [min(rpc, n_out - k * rpc) for k in range(n)]


def make_table(rng, kind, kv, n_in, n_out, first_chunk, last_chunk_start=0):
    """host-built tables: about half the entries -1, then the shape under test -- on tap kv // 2 where it is about one tap"""
    nbr = rng.integers(0, n_in, size=(kv, n_out)).astype(np.int32)
    nbr[rng.random((kv, n_out)) < 0.5] = -1
    t = kv // 2
    some = lambda k: rng.integers(0, n_in, size=k).astype(np.int32)
    if kind == "tap_off":
        nbr[t] = -1
    elif kind == "one_pair_last_row":
        nbr[t] = -1
        nbr[t, n_out - 1] = n_in - 1
    elif kind.startswith("pairs"):               # exactly 31 / 32 / 33 pairs, all inside the first chunk
        k = int(kind[5:])
        nbr[t] = -1
        nbr[t, rng.choice(min(first_chunk, n_out), size=k, replace=False)] = some(k)
    elif kind == "dense":
        nbr[t] = some(n_out)
    elif kind == "ring287":                      # 31 pairs in the first 256 rows, then a dense 256-row block: 287 pairs in the ring
        assert n_out >= 512
        nbr[t] = -1
        nbr[t, rng.choice(256, size=31, replace=False)] = some(31)
        nbr[t, 256:512] = some(256)
    elif kind == "last_chunk":
        assert 0 < last_chunk_start < n_out
        nbr[:, :last_chunk_start] = -1
    elif kind == "empty3":                       # three empty 256-row blocks, then pairs
        assert n_out > 768
        nbr[:, :768] = -1
    elif kind == "one_row":
        nbr[:] = n_in // 2
    elif kind == "last_row":
        nbr[:, n_out - 1] = n_in - 1
    else:
        assert kind == "rand"
    return nbr


def wgrad_inputs(fam, rng, n_in, n_out, data):
    if data == "exact":
        return dyadic(rng, (n_in, fam.c_in)), dyadic(rng, (n_out, fam.c_out))
    # the wide dynamic range of test_wgrad_split_bf16_is_fp32_equivalent: full mantissas, row scales over several decades
    x = (rng.normal(size=(n_in, fam.c_in)) * np.exp(rng.normal(size=(n_in, 1)) * 2)).astype(np.float32)
    return x, rng.normal(size=(n_out, fam.c_out)).astype(np.float32)


def launch(fam, mp, label, *, n_in, n_out, kv, nbr, pitches=None, data="exact", accumulate=False, misalign=False, wgs=None, absmax=True, seed=0,
           f16_floor=False):
    """One T.conv_wgrad launch of `fam` with every check of this file -> (dw fp32 numpy, dict(kernel, rpc, n_chunks) of the launch).
    nbr: host table [kv, n_out], or None with kv = 1."""
    for k in KNOBS:
        mp.delenv(k, raising=False)
    if wgs is not None:                          # the planner's speed-only knobs are read under CPD_TUNE=1 alone
        mp.setenv("CPD_TUNE", "1")
        mp.setenv("CPD_WGRAD_WGS", str(wgs))
    rng = np.random.default_rng(seed + 7919 * n_out + 31 * kv + n_in)
    c_in, c_out = fam.c_in, fam.c_out
    p_x, p_dy = pitches or fam.pitches
    assert n_in != n_out and n_out <= 1536
    if nbr is not None:
        assert nbr.shape == (kv, n_out) and nbr.min() >= -1 and nbr.max() < n_in      # never an out-of-range index
    else:
        assert kv == 1 and n_in > n_out
    x_np, dy_np = wgrad_inputs(fam, rng, n_in, n_out, data)
    x, dy = in_buffer(x_np, p_x), in_buffer(dy_np, p_dy)
    dw = Flat((kv, c_in, c_out), c_in * c_out, misalign)
    dw0 = None
    if accumulate:
        dw0 = dyadic(rng, (kv, c_in, c_out))
        dw.view.copy_(torch.from_numpy(dw0).cuda())
    kw = {}
    if fam.kind in SPLIT:
        kw["math"] = "bf16x3" if fam.kind == "bf16" else "f16x2"
        if fam.kind == "f16" and absmax:
            kw.update(in_absmax=T.absmax_block(x), dy_absmax=T.absmax_block(dy))
    nbr_dev = torch.from_numpy(nbr).cuda() if nbr is not None else None
    with ops.launch_log() as log:
        out = T.conv_wgrad(x, c_in, dy, c_out, nbr_dev, kv, n_out, dw=dw.view, accumulate=accumulate, **kw)
    torch.cuda.synchronize()
    assert out is dw.view
    LOGGED.update(log.counts)

    # ---- which kernel ran
    want_log = {expected_kernel(fam, x, dy): 1}
    assert log.counts == want_log, (label, log.counts, want_log)
    rpc, n_chunks = plan(fam, n_out, kv, wgs)

    # ---- what it wrote, and what it left alone
    got = dw.check(label)
    assert np.isfinite(got).all(), (label, "NaN / inf in dw: a padding column or a row past n_in / n_out reached an accumulator",
                                    np.argwhere(~np.isfinite(got))[:8].tolist())
    ref, pairs, S = R.wgrad_ref(x_np, dy_np, nbr, n_out)
    if data == "exact":
        # premise: at most 1536 pairs of multiples of 1/64 no larger than 4, so |any partial sum| * 64 < 2^24
        assert pairs.max() <= 1536 and (S.max() + 2) * 64 < 2 ** 24, (label, pairs.max(), S.max())
        if accumulate:
            ref = ref + dw0
        assert np.array_equal(ref * 64, np.rint(ref * 64)), label
        want = exactly_representable(ref, label)
        wrong = np.argwhere(got != want)
        assert wrong.size == 0, (label, "dw differs from the exact sum at (tap, ci, co)", wrong[:8].tolist(),
                                 [(float(got[tuple(i)]), float(want[tuple(i)])) for i in wrong[:8]], "pairs per tap", pairs.tolist(),
                                 "chunks", n_chunks, "of", rpc)
    else:
        assert not accumulate
        # worst-case fp32 summation of pairs[t] products and n_chunks partials; the factor 2 covers the roundings inside one MFMA
        # step and the split's own residual
        bound = 2.0 * (pairs[:, None, None] + n_chunks + 2) * U * S
        if f16_floor and fam.kind == "f16":
            bound = bound + f16_floor_term(x_np, dy_np, nbr, n_out)
        err = np.abs(got.astype(np.float64) - ref)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        assert (err <= bound).all(), (label, "beyond the fp32 summation bound at (tap, ci, co)", [int(i) for i in worst], "error", float(err[worst]),
                                      "bound", float(bound[worst]), "pairs", int(pairs[worst[0]]))
    return got, dict(kernel=next(iter(log.counts)), rpc=rpc, n_chunks=n_chunks)


def f16_floor_term(x, dy, nbr, n_out):
    """What the fp16 pair cannot hold, per element of dw: an operand is scaled by s = 2^(14 - floor(log2 max |operand|)) and split
    into two fp16 terms, the low one with fp16's smallest spacing 2^-24 -- an ABSOLUTE error of up to 2^-25 / s per entry, which is
    more than 2^-24 relative for entries below max / 2^18. Summed over a tap's pairs: q_x . sum |dy| + q_dy . sum |x|."""
    qx, qdy = (2.0 ** (np.floor(np.log2(np.abs(a).max())) - 14 - 25) for a in (x, dy[:n_out]))
    out = np.zeros((nbr.shape[0], x.shape[1], dy.shape[1]))
    for t in range(nbr.shape[0]):
        j = np.flatnonzero(nbr[t] >= 0)
        out[t] = qx * np.abs(dy[j]).sum(0, dtype=np.float64)[None, :] + qdy * np.abs(x[nbr[t, j]]).sum(0, dtype=np.float64)[:, None]
    return out


def n_in_for(n_out):
    return 300 if n_out < 100 else 41            # apart from n_out either way


WAVE_ROWS = (1, 3, 4, 5, 63, 64, 65, 257, 513)
TILE_ROWS = (1, 15, 16, 17, 129, 257)
SPLIT_ROWS = (1, 31, 32, 33, 255, 256, 257, 513)
# chunk structures of the row sweep (27 taps, default chunking), worked out by hand from the three plans
CHUNKS = {("wave", 257): [192, 65], ("wave", 513): [192, 192, 129], ("tile", 129): [80, 49], ("tile", 257): [96, 96, 65],
          ("split", 257): [256, 1], ("split", 513): [256, 256, 1], ("split", 255): [255], ("tile", 17): [17], ("wave", 65): [65]}


def row_sweep(fam):
    if fam.kind in SPLIT:
        return SPLIT_ROWS
    return TILE_ROWS if fam.c_in % 64 == 0 and fam.c_out % 64 == 0 else WAVE_ROWS


@gpu
@pytest.mark.parametrize("fam,n_out", [pytest.param(f, n, id="%s-n%d" % (f.key, n)) for f in FAMILIES for n in row_sweep(f)])
def test_wgrad_row_counts_around_stage_block_and_chunk(hip, monkeypatch, fam, n_out):
    """n_out at 1, around the 4-row step / 16-row stage / 32-pair stage, around the 64-row load / 256-row block, and at counts
    that leave a ragged last chunk. Exact data, compared for equality; dw once 16-byte aligned and overwritten, once 4 bytes
    further (the scalar form of the chunk sum) and accumulated into."""
    kind = "split" if fam.kind in SPLIT else ("tile" if row_sweep(fam) is TILE_ROWS else "wave")
    if (kind, n_out) in CHUNKS:
        assert chunk_rows(fam, n_out, 27) == CHUNKS[(kind, n_out)], (fam.key, n_out, chunk_rows(fam, n_out, 27))
    n_in = n_in_for(n_out)
    rng = np.random.default_rng(n_out)
    first = plan(fam, n_out, 27)[0]
    for table, acc, mis in (("rand", False, False), ("last_row", True, True), ("rand", True, False), ("last_row", False, True)):
        nbr = make_table(rng, table, 27, n_in, n_out, first)
        launch(fam, monkeypatch, (fam.key, "n_out", n_out, table, "accumulate", acc, "misaligned dw", mis), n_in=n_in, n_out=n_out, kv=27, nbr=nbr,
               accumulate=acc, misalign=mis)


@gpu
@pytest.mark.parametrize("fam", [f for f in FAMILIES if f.kind in SPLIT], ids=str)
def test_wgrad_ring_wraps_in_one_long_chunk(hip, monkeypatch, fam):
    """1300 rows as ONE chunk (CPD_WGRAD_WGS=1) of six 256-row blocks: a dense tap pushes 1300 pairs through the 512-entry ring"""
    n_out, n_in = 1300, 41
    assert chunk_rows(fam, n_out, 27, wgs=1) == [1300]
    rng = np.random.default_rng(13)
    for table in ("dense", "rand"):
        nbr = make_table(rng, table, 27, n_in, n_out, 1300)
        launch(fam, monkeypatch, (fam.key, "one chunk of 1300", table), n_in=n_in, n_out=n_out, kv=27, nbr=nbr, wgs=1, accumulate=table == "rand")


TABLES = ("rand", "tap_off", "one_pair_last_row", "pairs31", "pairs32", "pairs33", "dense", "ring287", "last_chunk", "empty3", "one_row")


def table_rows(fam, table):
    """(n_out, CPD_WGRAD_WGS or None) of a table case: one mid-size count per family that has more than one chunk; the two ring
    shapes need 512 / more than 768 rows in ONE chunk, which the split kernels get from the knob"""
    split = fam.kind in SPLIT
    if table == "ring287":
        return 600, (1 if split else None)
    if table == "empty3":
        return 900, (1 if split else None)
    return (513 if split else (129 if fam.c_in % 64 == 0 and fam.c_out % 64 == 0 else 257)), None


@gpu
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("fam", FAMILIES, ids=str)
def test_wgrad_table_shapes(hip, monkeypatch, fam, table):
    n_out, wgs = table_rows(fam, table)
    n_in = 41
    rpc, n_chunks = plan(fam, n_out, 27, wgs)
    if wgs:
        assert n_chunks == 1
    elif table not in ("ring287", "empty3"):
        assert n_chunks > 1
    nbr = make_table(np.random.default_rng(len(table) + n_out), table, 27, n_in, n_out, rpc, (n_chunks - 1) * rpc)
    for acc in (False, True):
        got, _ = launch(fam, monkeypatch, (fam.key, table, "accumulate", acc), n_in=n_in, n_out=n_out, kv=27, nbr=nbr, accumulate=acc, wgs=wgs)
        if table == "tap_off" and not acc:       # (under accumulate the slice must be the old dw: the equality in launch() says so)
            assert not got[13].any() and not np.signbit(got[13]).any(), (fam.key, "the slice of a tap without pairs is not +0")


@gpu
@pytest.mark.parametrize("kv", [0, 1, 9, 27], ids=lambda k: "kv%s" % (k or "1_no_table"))
@pytest.mark.parametrize("fam", FAMILIES, ids=str)
def test_wgrad_tap_counts(hip, monkeypatch, fam, kv):
    """kv = 1 without a table (output row j pairs with input row j), and tables of 1, 9 and 27 taps"""
    n_out, _ = table_rows(fam, "rand")
    if kv == 0:
        launch(fam, monkeypatch, (fam.key, "kv 1, no table"), n_in=n_out + 5, n_out=n_out, kv=1, nbr=None)
        launch(fam, monkeypatch, (fam.key, "kv 1, no table, accumulate"), n_in=n_out + 5, n_out=n_out, kv=1, nbr=None, accumulate=True, misalign=True)
        return
    nbr = make_table(np.random.default_rng(kv), "rand", kv, 41, n_out, plan(fam, n_out, kv)[0])
    launch(fam, monkeypatch, (fam.key, "kv", kv), n_in=41, n_out=n_out, kv=kv, nbr=nbr)
    launch(fam, monkeypatch, (fam.key, "kv", kv, "accumulate"), n_in=41, n_out=n_out, kv=kv, nbr=nbr, accumulate=True, misalign=True)


PITCHES = [(a, b) for k in ("wide32", "pad4", "odd") for a, b in ((k, "tight"), ("tight", k), (k, k))]


@gpu
@pytest.mark.parametrize("pitches", PITCHES, ids=lambda p: "x_%s-dy_%s" % p)
@pytest.mark.parametrize("fam", [f for f in FAMILIES if f.pitches == ("tight", "tight")], ids=str)
def test_wgrad_pitch_and_alignment(hip, monkeypatch, fam, pitches):
    """x and dy as views [rows, off : off + c] of wider buffers, independently. A view one float into its buffer (pitch c + 3) on
    either side routes a tile launch to the wave kernel (asserted from the launch log in launch()); the split kernels, which load
    element-wise, keep their instantiation"""
    n_out, _ = table_rows(fam, "rand")
    nbr = make_table(np.random.default_rng(len(pitches[0]) + 3 * len(pitches[1])), "last_row", 27, 41, n_out, 0)
    launch(fam, monkeypatch, (fam.key, pitches), n_in=41, n_out=n_out, kv=27, nbr=nbr, pitches=pitches)
    _, info = launch(fam, monkeypatch, (fam.key, pitches, "accumulate"), n_in=41, n_out=n_out, kv=27, nbr=nbr, pitches=pitches, accumulate=True,
                     misalign=True)
    if fam.kind == "tile":
        assert info["kernel"] == ("wgrad_kernel<4,4>" if "odd" in pitches else "wgrad_tile_kernel<%d,%d>" % (fam.c_in, fam.c_out)), (fam.key, pitches, info)
    if fam.kind in SPLIT:
        assert info["kernel"].startswith("wgrad_%s_kernel<" % fam.kind), (fam.key, pitches, info)


@gpu
@pytest.mark.parametrize("fam", FAMILIES, ids=str)
def test_wgrad_full_mantissa_within_the_fp32_summation_bound(hip, monkeypatch, fam):
    """Full-mantissa operands (x over several decades, dy normal) against float64 under
    |got - ref| <= 2 (pairs[t] + n_chunks + 2) 2^-24 S[t, ci, co] per element. This is the check that sees a wrong product pairing
    or a lost middle term of the split arithmetic (2^-8 S), which exact data cannot; at the 250 pairs per tap of this table it
    does NOT see a lost low term (2^-17 S against a bound of 2^-15 S) -- the next test does. Twice the same launch: bitwise equal
    (the chunk sum has a fixed order)."""
    n_out = 513 if fam.kind in SPLIT else 257
    n_in = 300
    assert plan(fam, n_out, 27)[1] > 1
    nbr = make_table(np.random.default_rng(5), "rand", 27, n_in, n_out, 0)
    a, _ = launch(fam, monkeypatch, (fam.key, "full mantissa"), n_in=n_in, n_out=n_out, kv=27, nbr=nbr, data="full")
    b, _ = launch(fam, monkeypatch, (fam.key, "full mantissa, again"), n_in=n_in, n_out=n_out, kv=27, nbr=nbr, data="full")
    assert np.array_equal(bits(a), bits(b)), (fam.key, "two runs of one launch differ")


FEW_PAIRS = (1, 2, 3, 4, 5, 8, 12, 16)


@gpu
@pytest.mark.parametrize("fam", FAMILIES, ids=str)
def test_wgrad_full_mantissa_on_taps_with_few_pairs(hip, monkeypatch, fam):
    """The same data and bound on a table whose first eight taps have 1 ... 16 pairs. The bound grows like pairs . S -- pairs^2 --
    and a lost low term of a split like sqrt(pairs): on the random table above (about 250 pairs per tap) the bound is 2^-15 S
    and cannot see a lost term of 2^-17 S; at one pair it is 12 . 2^-24 S and does. The fp16 split is held to the same bound plus
    what its number format cannot hold on this data (f16_floor_term): x spans more than the 2^18 between its largest entry and
    the entries an fp16 pair still resolves to 2^-24."""
    n_out = 513 if fam.kind in SPLIT else 257
    n_in = 300
    rng = np.random.default_rng(8)
    nbr = make_table(rng, "rand", 27, n_in, n_out, 0)
    for t, k in enumerate(FEW_PAIRS):
        nbr[t] = -1
        nbr[t, rng.choice(n_out, size=k, replace=False)] = rng.integers(0, n_in, size=k)
    assert (nbr >= 0).sum(1)[:len(FEW_PAIRS)].tolist() == list(FEW_PAIRS)
    launch(fam, monkeypatch, (fam.key, "full mantissa, few pairs"), n_in=n_in, n_out=n_out, kv=27, nbr=nbr, data="full", f16_floor=True)


@gpu
@pytest.mark.parametrize("fam", [f for f in FAMILIES if f.kind == "f16"], ids=str)
def test_wgrad_f16_without_absmax_blocks(hip, monkeypatch, fam):
    """the fp16 split without its pre-scale: |x| <= 2 needs none, and k / 8 splits exactly"""
    nbr = make_table(np.random.default_rng(6), "rand", 27, 41, 513, 0)
    launch(fam, monkeypatch, (fam.key, "no absmax blocks"), n_in=41, n_out=513, kv=27, nbr=nbr, absmax=False)


# ------------------------------------------------------------------------------------------------ B4: the workspace promise
def wgrad_direct(fam, mp, label, n_out, ws_short=0, kv=27, n_in=41):
    """lib().cpd_conv_wgrad_scaled with a workspace of exactly cpd_conv_wgrad_workspace_bytes(...) - ws_short bytes inside a
    pattern buffer, default chunking -> (rc, dw Flat, ws buffer [int32 words], ws words, reference fp32)"""
    for k in KNOBS:
        mp.delenv(k, raising=False)
    rng = np.random.default_rng(n_out + fam.c_in)
    nbr = make_table(rng, "rand", kv, n_in, n_out, 0)
    x_np, dy_np = wgrad_inputs(fam, rng, n_in, n_out, "exact")
    x, dy = in_buffer(x_np, fam.pitches[0]), in_buffer(dy_np, fam.pitches[1])
    dw = Flat((kv, fam.c_in, fam.c_out), fam.c_in * fam.c_out)
    ws_bytes = lib().cpd_conv_wgrad_workspace_bytes(n_out, fam.c_in, fam.c_out, kv)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws = torch.full((ws_bytes // 4 + 1024,), PATTERN, dtype=torch.int32, device="cuda")
    assert ws.data_ptr() % 256 == 0
    flags = {"bf16": 2, "f16": 4}.get(fam.kind, 0)
    blocks = (T.absmax_block(x), T.absmax_block(dy)) if fam.kind == "f16" else (None, None)
    nbr_dev = torch.from_numpy(nbr).cuda()
    with ops.launch_log() as log:
        rc = lib().cpd_conv_wgrad_scaled(vp(x), x.stride(0), fam.c_in, vp(dy), dy.stride(0), fam.c_out, vp(nbr_dev), kv, n_out, vp(dw.view), flags,
                                         vp(blocks[0]), vp(blocks[1]), vp(ws), ws_bytes - ws_short, stream())
    torch.cuda.synchronize()
    if rc == 0:
        assert log.counts == {expected_kernel(fam, x, dy): 1}, (label, log.counts)
    else:
        assert log.counts == {}, (label, log.counts)
    want = exactly_representable(R.wgrad_ref(x_np, dy_np, nbr, n_out)[0], label)
    return rc, dw, ws, ws_bytes // 4, want


WS_FAMS = ["wave_40_33", "wave_5_7", "tile_64_128", "tile_128_128", "bf16_64_64", "bf16_32_128", "f16_128_32", "f16_192_64", "wave_misaligned_64_64"]


@gpu
@pytest.mark.parametrize("n_out", [65, 257, 513, 1300])
@pytest.mark.parametrize("key", WS_FAMS)
def test_wgrad_fits_the_workspace_it_asks_for(hip, monkeypatch, key, n_out):
    """cpd_conv_wgrad_workspace_bytes is a promise: a workspace of exactly that size is enough for whichever plan the flags
    select -- the wave plan, the tile plan, the tile plan run by the wave kernel, either split plan -- and no word behind it is
    written"""
    fam = next(f for f in FAMILIES if f.key == key)
    rc, dw, ws, words, want = wgrad_direct(fam, monkeypatch, (key, n_out), n_out)
    assert rc == 0, (key, n_out, rc)
    got = dw.check((key, n_out))
    assert np.array_equal(got, want), (key, n_out, np.argwhere(got != want)[:8].tolist())
    behind = ws[words:].cpu().numpy()
    assert (behind == PATTERN).all(), (key, n_out, "wrote behind its workspace at words", np.flatnonzero(behind != PATTERN)[:8].tolist())
    need = plan(fam, n_out, 27)[1] * 27 * fam.c_in * fam.c_out
    assert need <= words, (key, n_out, "the plan restated here needs more than the library promises", need, words)


@gpu
@pytest.mark.parametrize("key,n_out", [("tile_64_64", 513), ("bf16_32_32", 513), ("wave_misaligned_64_64", 513), ("f16_32_32", 257)])
def test_wgrad_refuses_a_workspace_one_byte_short(hip, monkeypatch, key, n_out):
    """shapes whose plan needs every byte of the promise (no rounding slack, no larger other plan): one byte less is
    CPD_ERR_WORKSPACE, before anything is launched or written"""
    fam = next(f for f in FAMILIES if f.key == key)
    rc, dw, ws, words, _ = wgrad_direct(fam, monkeypatch, (key, "one byte short"), n_out, ws_short=1)
    assert plan(fam, n_out, 27)[1] * 27 * fam.c_in * fam.c_out == words, "this shape leaves slack: not a case for this test"
    assert rc == -2, (key, rc)                    # CPD_ERR_WORKSPACE
    assert dw.untouched() and bool((ws == PATTERN).all()), key


@gpu
@pytest.mark.parametrize("key", ["wave_5_7", "tile_64_64", "bf16_32_32", "f16_64_64"])
def test_wgrad_refuses_zero_rows(hip, monkeypatch, key):
    fam = next(f for f in FAMILIES if f.key == key)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    x, dy = in_buffer(np.ones((5, fam.c_in), np.float32), "tight"), in_buffer(np.ones((5, fam.c_out), np.float32), "tight")
    dw = Flat((27, fam.c_in, fam.c_out), fam.c_in * fam.c_out)
    nbr = torch.zeros((27, 5), dtype=torch.int32, device="cuda")
    kw = {"math": {"bf16": "bf16x3", "f16": "f16x2"}[fam.kind]} if fam.kind in SPLIT else {}
    with ops.launch_log() as log:
        with pytest.raises(CpdHipError):
            T.conv_wgrad(x, fam.c_in, dy, fam.c_out, nbr, 27, 0, dw=dw.view, **kw)
    torch.cuda.synchronize()
    assert log.counts == {} and dw.untouched(), (key, log.counts)


@gpu
def test_every_weight_gradient_instantiation_is_reached(hip, monkeypatch):
    """one launch per family spec: the logged names are all 9 + 4 + 9 + 9 instantiations, and nothing else"""
    seen = set()
    for fam in FAMILIES:
        nbr = make_table(np.random.default_rng(9), "rand", 27, 41, 65, 0)
        seen.add(launch(fam, monkeypatch, (fam.key, "coverage"), n_in=41, n_out=65, kv=27, nbr=nbr)[1]["kernel"])
    print("instantiations logged:", *sorted(seen), sep="\n  ")
    assert seen == ALL_NAMES, (sorted(ALL_NAMES - seen), sorted(seen - ALL_NAMES))
    assert LOGGED <= ALL_NAMES, sorted(LOGGED - ALL_NAMES)


# ================================================================================================ C. column reductions, row kernels
C_SWEEP = (1, 3, 4, 5, 60, 64, 68, 320)
N_SWEEP = (1, 2, 63, 64, 65, 1025, 4097)
SHAPES = [pytest.param(c, n, p, id="c%d-n%d-%s" % (c, n, p)) for c in C_SWEEP for n in N_SWEEP for p in ("tight", "wide32", "odd")]


def col_plan(n, c, vec, col_blocks=256):
    """col_reduce's launch, restated -> dict(V, cq, rl, col_tiles, chunks, rpc): a block is cq column groups (of V columns) x rl
    row lanes; a thread adds every rl-th row of its chunk, then row lane 0 adds the rl lanes' sums, all in fp32"""
    V = 4 if vec else 1
    cq_total = cdiv(c, V)
    cq = min(cq_total, 16)
    rl = 256 // cq
    col_tiles = cdiv(cq_total, cq)
    chunks = max(1, min(col_blocks // col_tiles, cdiv(n, 4 * rl), 512))
    rpc = cdiv(cdiv(n, chunks), rl) * rl
    return dict(V=V, cq=cq, rl=rl, col_tiles=col_tiles, chunks=cdiv(n, rpc), rpc=rpc)


def clear_knobs(mp):
    for k in KNOBS:
        mp.delenv(k, raising=False)


def test_the_sweep_reaches_the_column_group_shapes_it_is_meant_to():
    """c = 3 and 5 give fewer than 16 column groups with 256 / cq = 85 and 51 row lanes (not powers of two, one idle thread); 60
    gives 15 groups of 4 (17 lanes, one idle); 68 a second column tile with one group; an odd pitch turns the vector form off"""
    assert [col_plan(65, c, False)[k] for c in (3, 5) for k in ("cq", "rl")] == [3, 85, 5, 51]
    assert (col_plan(65, 60, True)["cq"], col_plan(65, 60, True)["rl"]) == (15, 17)
    assert (col_plan(65, 68, True)["col_tiles"], col_plan(65, 64, True)["col_tiles"]) == (2, 1)
    assert col_plan(65, 64, False)["col_tiles"] == 4 and col_plan(65, 320, True)["col_tiles"] == 5


@gpu
@pytest.mark.parametrize("c,n,pitch", SHAPES)
def test_column_sums_are_exact(hip, monkeypatch, c, n, pitch):
    """col_sum and both outputs of bn_stats on k / 8 data: |sum| <= 8194 in multiples of 1/8 and sum x^2 <= 16388 in multiples of
    1/64 are fp32 numbers whatever the order of the additions, so they must EQUAL the float64 sums"""
    clear_knobs(monkeypatch)
    rng = np.random.default_rng(c * 10007 + n)
    x_np = dyadic(rng, (n, c))
    x = in_buffer(x_np, pitch)
    want1, want2 = (exactly_representable(a, (c, n, pitch)) for a in R.bn_ref.stats(x_np))
    out = Flat((c,), c, misalign=pitch == "odd")
    assert T.col_sum(x, out=out.view) is out.view
    s1, s2 = T.bn_stats(x)
    torch.cuda.synchronize()
    got = out.check(("col_sum", c, n, pitch))
    assert np.array_equal(got, want1), ("col_sum", np.flatnonzero(got != want1)[:8].tolist(), got[:4], want1[:4])
    assert np.array_equal(s1.cpu().numpy(), want1), ("bn_stats sum", np.flatnonzero(s1.cpu().numpy() != want1)[:8].tolist())
    assert np.array_equal(s2.cpu().numpy(), want2), ("bn_stats sumsq", np.flatnonzero(s2.cpu().numpy() != want2)[:8].tolist())


@gpu
@pytest.mark.parametrize("c,pitch", [(320, "tight"), (64, "odd"), (5, "tight")])
def test_column_sums_with_the_most_chunks(hip, monkeypatch, c, pitch):
    """CPD_COL_BLOCKS=512 (under CPD_TUNE=1): as many row chunks as the four-rows-per-thread floor allows, the last one ragged"""
    n = 4097
    p = col_plan(n, c, pitch == "tight" and c % 4 == 0, 512)
    assert p["chunks"] == cdiv(n, 4 * p["rl"]) >= col_plan(n, c, pitch == "tight" and c % 4 == 0)["chunks"] and n % p["rpc"] != 0, p
    clear_knobs(monkeypatch)
    monkeypatch.setenv("CPD_TUNE", "1")
    monkeypatch.setenv("CPD_COL_BLOCKS", "512")
    rng = np.random.default_rng(c)
    x_np, g_np = dyadic(rng, (n, c)), dyadic(rng, (n, c))
    x, g = in_buffer(x_np, pitch), in_buffer(g_np, pitch)
    want1, want2 = (exactly_representable(a, c) for a in R.bn_ref.stats(x_np))
    s1, s2 = T.bn_stats(x)
    assert np.array_equal(s1.cpu().numpy(), want1) and np.array_equal(s2.cpu().numpy(), want2)
    assert np.array_equal(T.col_sum(g).cpu().numpy(), exactly_representable(R.bn_ref.col_sum(g_np), c))
    bn_backward_case(c, n, pitch, rng)


def dx_bound(x, mean, invstd, gamma, gm, dbeta, dgamma):
    """8 . 2^-24 . |gamma . invstd| . (|g_m| + |dbeta| / n + |xhat . dgamma| / n): four fp32 operations and the rounding of 1 / n,
    relative to the magnitudes that enter them"""
    n = x.shape[0]
    xhat = (x.astype(np.float64) - mean) * invstd
    return 8 * U * np.abs(gamma.astype(np.float64) * invstd) * (np.abs(gm) + np.abs(dbeta) / n + np.abs(xhat * dgamma) / n)


def bn_backward_case(c, n, pitch, rng, with_y=True):
    """cpd_bn_bwd_reduce + cpd_bn_bwd_apply on exact data, every output a guarded view"""
    label = ("bn_backward", c, n, pitch, "relu" if with_y else "no relu")
    x_np, g_np = dyadic(rng, (n, c)), dyadic(rng, (n, c))
    y_np = rng.choice(np.array([0.0, -0.0, -1.5, -0.125, 0.25, 2.0], np.float32), size=(n, c)) if with_y else None
    mean_np = dyadic(rng, (c,))
    invstd_np = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=c)
    gamma_np = rng.uniform(0.5, 1.5, c).astype(np.float32)
    x, g = in_buffer(x_np, pitch), in_buffer(g_np, pitch)
    y = in_buffer(y_np, pitch) if with_y else None
    dev = lambda a: torch.from_numpy(a).cuda()
    mean, invstd, gamma = dev(mean_np), dev(invstd_np), dev(gamma_np)
    sums = Flat((2, c), c, misalign=pitch == "odd")
    dbeta, dgamma = sums.view[0], sums.view[1]
    dx, dres = Rows(n, c, pitch), Rows(n, c, pitch)
    block = torch.zeros(T.ABSMAX_WORDS, dtype=torch.int32, device="cuda")
    ws = T._ws(lib().cpd_col_reduce_workspace_bytes(n, c), "cuda")
    ldy = y.stride(0) if with_y else 0
    rc = lib().cpd_bn_bwd_reduce(vp(g), g.stride(0), vp(y), ldy, vp(x), x.stride(0), vp(mean), vp(invstd), n, c, vp(dbeta), vp(dgamma), vp(ws),
                                 ws.numel(), stream())
    assert rc == 0, (label, rc)
    rc = lib().cpd_bn_bwd_apply(vp(g), g.stride(0), vp(y), ldy, vp(x), x.stride(0), n, c, vp(mean), vp(invstd), vp(gamma), vp(dbeta), vp(dgamma),
                                vp(dx.view), dx.view.stride(0), vp(dres.view), dres.view.stride(0), vp(block), stream())
    assert rc == 0, (label, rc)
    torch.cuda.synchronize()
    ref_dx, ref_dgamma, ref_dbeta, ref_dres = R.bn_ref.backward(g_np, y_np, x_np, mean_np, invstd_np, gamma_np)
    got_sums = sums.check(label)
    # xhat and g . xhat are multiples of 1/128 no larger than 16: the sums of up to 4097 of them are fp32 numbers
    assert np.array_equal(got_sums[0], exactly_representable(ref_dbeta, label)), (label, "dbeta", got_sums[0][:4], ref_dbeta[:4])
    assert np.array_equal(got_sums[1], exactly_representable(ref_dgamma, label)), (label, "dgamma", got_sums[1][:4], ref_dgamma[:4])
    got_dres, got_dx = dres.check(label + ("dres",)), dx.check(label + ("dx",))
    assert np.array_equal(bits(got_dres), bits(ref_dres.astype(np.float32))), (label, "dres")
    assert np.isfinite(got_dx).all(), (label, "NaN / inf in dx")
    bound = dx_bound(x_np, mean_np, invstd_np, gamma_np, ref_dres, ref_dbeta, ref_dgamma)
    err = np.abs(got_dx.astype(np.float64) - ref_dx)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), (label, "dx at", [int(i) for i in worst], float(err[worst]), float(bound[worst]))
    assert np.float32(ops.absmax_value(block)) == np.abs(got_dx).max(), (label, "dx_absmax", ops.absmax_value(block), float(np.abs(got_dx).max()))


@gpu
@pytest.mark.parametrize("c,n,pitch", SHAPES)
def test_bn_backward_sums_are_exact_and_dx_is_within_rounding(hip, monkeypatch, c, n, pitch):
    clear_knobs(monkeypatch)
    rng = np.random.default_rng(c * 7919 + n)
    bn_backward_case(c, n, pitch, rng)
    if n <= 65:
        bn_backward_case(c, n, pitch, rng, with_y=False)


@gpu
def test_bn_backward_with_one_misaligned_operand(hip, monkeypatch):
    """c = 64, every operand aligned but one -- each in turn: the scalar forms must be chosen (a vector access at a 4-byte offset
    faults or reads the neighbour's columns), through T.bn_backward / T.affine_rows / T.relu_backward as the trainer calls them"""
    clear_knobs(monkeypatch)
    n, c = 65, 64
    rng = np.random.default_rng(1)
    g_np, x_np, r_np = dyadic(rng, (n, c)), dyadic(rng, (n, c)), dyadic(rng, (n, c))
    y_np = rng.choice(np.array([0.0, -0.0, -1.5, 2.0], np.float32), size=(n, c))
    mean_np, invstd_np = dyadic(rng, (c,)), rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=c)
    gamma_np = rng.choice(np.array([0.5, 1.0, 1.5], np.float32), size=c)
    dev = lambda a: torch.from_numpy(a).cuda()
    ref_dx, ref_dgamma, ref_dbeta, ref_dres = R.bn_ref.backward(g_np, y_np, x_np, mean_np, invstd_np, gamma_np)
    ref_aff = R.bn_ref.affine(x_np, gamma_np, mean_np, r_np, True).astype(np.float32)
    for odd in range(3):
        p = ["odd" if i == odd else "tight" for i in range(3)]
        g, y, x = in_buffer(g_np, p[0]), in_buffer(y_np, p[1]), in_buffer(x_np, p[2])
        dx, dgamma, dbeta, dres = T.bn_backward(g, y, x, dev(mean_np), dev(invstd_np), dev(gamma_np), want_dres=True)
        assert np.array_equal(dbeta.cpu().numpy(), ref_dbeta.astype(np.float32)) and np.array_equal(dgamma.cpu().numpy(), ref_dgamma.astype(np.float32)), p
        assert np.array_equal(bits(dres.cpu().numpy()), bits(ref_dres.astype(np.float32))), p
        assert (np.abs(dx.cpu().numpy().astype(np.float64) - ref_dx) <= dx_bound(x_np, mean_np, invstd_np, gamma_np, ref_dres, ref_dbeta, ref_dgamma)).all(), p
        assert np.array_equal(bits(T.relu_backward(g, y).cpu().numpy()), bits(R.bn_ref.relu_backward(g_np, y_np).astype(np.float32))), p
        xa, ra = in_buffer(x_np, p[0]), in_buffer(r_np, p[1])
        out = Rows(n, c, p[2])
        T.affine_rows(xa, dev(gamma_np), dev(mean_np), ra, True, out=out.view)
        assert np.array_equal(bits(out.check(("affine", p))), bits(ref_aff)), p


AFFINE = {"all": (1, 1, 1, 1), "no_scale": (0, 1, 1, 1), "no_shift": (1, 0, 1, 1), "no_residual": (1, 1, 0, 1), "no_relu": (1, 1, 1, 0),
          "none": (0, 0, 0, 0), "relu": (0, 0, 0, 1), "scale": (1, 0, 0, 0)}


@gpu
@pytest.mark.parametrize("c,n,pitch", SHAPES)
def test_affine_rows_and_relu_backward_to_the_bit(hip, monkeypatch, c, n, pitch):
    """scale in {0.5, 1, 1.5}, dyadic x / shift / residual: every intermediate is an fp32 number, so out must equal the reference
    bit for bit (fused or not); with and without each of scale, shift, residual and ReLU"""
    clear_knobs(monkeypatch)
    rng = np.random.default_rng(c * 104729 + n)
    x_np, r_np, g_np = dyadic(rng, (n, c)), dyadic(rng, (n, c)), dyadic(rng, (n, c))
    y_np = rng.choice(np.array([0.0, -0.0, -1.5, -0.125, 0.25, 2.0], np.float32), size=(n, c))
    scale_np, shift_np = rng.choice(np.array([0.5, 1.0, 1.5], np.float32), size=c), dyadic(rng, (c,))
    x, res = in_buffer(x_np, pitch), in_buffer(r_np, pitch)
    ss = Flat((2, c), 4, misalign=pitch == "odd")
    ss.view.copy_(torch.from_numpy(np.stack([scale_np, shift_np])).cuda())
    for name, (s, b, r, relu) in AFFINE.items():
        out = Rows(n, c, pitch)
        T.affine_rows(x, ss.view[0] if s else None, ss.view[1] if b else None, res if r else None, bool(relu), out=out.view)
        want = R.bn_ref.affine(x_np, scale_np if s else None, shift_np if b else None, r_np if r else None, bool(relu))
        got = out.check(("affine_rows", name, c, n, pitch))
        assert np.array_equal(bits(got), bits(exactly_representable(want, name))), ("affine_rows", name, c, n, pitch, np.argwhere(got != want)[:8].tolist())
    g, y = in_buffer(g_np, pitch), in_buffer(y_np, pitch)
    dx = Rows(n, c, pitch)
    rc = lib().cpd_relu_bwd(vp(g), g.stride(0), vp(y), y.stride(0), n, c, vp(dx.view), dx.view.stride(0), stream())
    assert rc == 0
    got = dx.check(("relu_backward", c, n, pitch))
    assert np.array_equal(bits(got), bits(R.bn_ref.relu_backward(g_np, y_np).astype(np.float32))), ("relu_backward", c, n, pitch)


@gpu
@pytest.mark.parametrize("c,n,pitch", SHAPES)
def test_bn_stats_finalize_within_an_ulp(hip, monkeypatch, c, n, pitch):
    """mean, invstd, scale and shift within 1 ulp of the float64 formula rounded to fp32, the running statistics within 2.

    On k / 8 data the column sums are exact, so what is measured is the finalisation alone. Where the bounds come from: mean and
    invstd are one rounding of a double (<= 1 ulp with the double rounding); scale = gamma . fl(invstd) carries invstd's half ulp
    and its own: below 2 ulp against the rounded exact value, hence at most 1. shift = beta - mean . scale is held to an ulp OF
    THE RESULT, which no fp32 evaluation meets under cancellation: beta is drawn with the sign opposite to mean . scale and at
    least 8 times its size, so that the product's 1.5 ulp weigh less than a quarter ulp of the result. The momentum is 1/8 (1 - m
    and m . v are then exact) and the running mean starts with the sign of the batch mean (no cancellation): two roundings per
    running statistic, within the 2 ulp the check allows."""
    clear_knobs(monkeypatch)
    rng = np.random.default_rng(c * 15485863 + n)
    eps, momentum = np.float32(1e-3), 0.125
    x_np = dyadic(rng, (n, c))
    gamma_np = rng.uniform(0.5, 1.5, c).astype(np.float32)
    s1, s2 = R.bn_ref.stats(x_np)
    rm_np = (rng.uniform(0.5, 2.0, c) * np.where(s1 >= 0, 1.0, -1.0)).astype(np.float32)
    rv_np = rng.uniform(0.5, 2.0, c).astype(np.float32)
    pre = R.bn_ref.finalize(s1, s2, n, float(eps), momentum, gamma_np, np.zeros(c))
    ms = pre["mean"] * pre["scale"]
    beta_np = (-np.where(ms >= 0, 1.0, -1.0) * (8 * np.abs(ms) + rng.uniform(0.5, 1.5, c))).astype(np.float32)
    want = R.bn_ref.finalize(s1, s2, n, float(eps), momentum, gamma_np, beta_np, rm_np, rv_np)
    x = in_buffer(x_np, pitch)
    dev = lambda a: torch.from_numpy(a).cuda()
    rm, rv = dev(rm_np), dev(rv_np)
    got = dict(zip(("mean", "invstd", "scale", "shift"), T.bn_stats_finalize(x, float(eps), momentum, dev(gamma_np), dev(beta_np), rm, rv)))
    got.update(running_mean=rm, running_var=rv)
    if n == 1:
        assert not want["var"].any()             # one row: variance 0, and the running update keeps the biased value
    for key, tol in (("mean", 1), ("invstd", 1), ("scale", 1), ("shift", 1), ("running_mean", 2), ("running_var", 2)):
        g = got[key].cpu().numpy()
        d = ulps(g, want[key].astype(np.float32))
        assert np.isfinite(g).all() and d.max() <= tol, (key, c, n, pitch, "ulps", int(d.max()), "column", int(d.argmax()), float(g[d.argmax()]),
                                                         float(want[key][d.argmax()]))


# ================================================================================================ D. conditioning of the variance
@gpu
@pytest.mark.parametrize("ratio", [0, 8, 64])
def test_variance_of_fp32_sums_within_the_summation_bound(hip, monkeypatch, ratio):
    """Columns of standard deviation 1 and mean `ratio`, full-mantissa normal data, n = 4097, c = 64, tight rows: the variance that
    bn_stats implies (sumsq / n - mean^2) and the one behind bn_stats_finalize's invstd, against float64.

    The launch (col_plan): 16-byte loads, 16 column groups x 16 row lanes, 65 chunks of 64 rows. A thread adds 64 / 16 = 4 rows,
    row lane 0 then adds the 16 lanes' sums: the longest fp32 addition chain is L = 4 + 16 = 20 (the 65 chunk totals are added in
    double). The bound is the worst case of such a chain on the sum of squares, (L + 2) 2^-24 mean(x^2), the 2 for the square's
    own rounding and the result's. It says nothing about how many DIGITS of the variance survive: at mean / sigma = 64, mean(x^2)
    is 4097 times the variance. The measured relative errors are printed, and recorded in DESIGN.md."""
    clear_knobs(monkeypatch)
    n, c = 4097, 64
    p = col_plan(n, c, True)
    assert (p["V"], p["cq"], p["rl"], p["chunks"], p["rpc"]) == (4, 16, 16, 65, 64)
    L = p["rpc"] // p["rl"] + p["rl"]
    assert L == 20
    rng = np.random.default_rng(ratio)
    x_np = (rng.normal(size=(n, c)) + ratio).astype(np.float32)
    x64 = x_np.astype(np.float64)
    var64, msq = x64.var(0), (x64 * x64).mean(0)
    x = torch.from_numpy(x_np).cuda()
    s1, s2 = (a.cpu().numpy().astype(np.float64) for a in T.bn_stats(x))
    var_stats = s2 / n - (s1 / n) ** 2
    eps = np.float32(1e-3)
    ones = torch.ones(c, device="cuda")
    _, invstd, _, _ = T.bn_stats_finalize(x, float(eps), 0.1, ones, ones)
    invstd = invstd.cpu().numpy().astype(np.float64)
    var_fin = 1.0 / invstd ** 2 - float(eps)
    bound = (L + 2) * U * msq
    print("variance conditioning: mean/sigma %d: max relative error of the variance %.3e (bn_stats), %.3e (bn_stats_finalize); bound / variance %.3e"
          % (ratio, (np.abs(var_stats - var64) / var64).max(), (np.abs(var_fin - var64) / var64).max(), (bound / var64).max()))
    assert (np.abs(var_stats - var64) <= bound).all(), (ratio, float((np.abs(var_stats - var64) / bound).max()))
    # invstd is one more fp32 rounding: half an ulp of invstd is at most 2^-23 of (variance + eps)
    assert (np.abs(var_fin - var64) <= bound + 2 * U * (var64 + float(eps))).all(), (ratio, float((np.abs(var_fin - var64) / bound).max()))


# ================================================================================================ E. transposed tables
@gpu
@pytest.mark.parametrize("h,w,k,stride,pad", [(1, 1, 3, 1, 1), (5, 7, 3, 2, 1), (6, 6, 2, 2, 0), (7, 5, 3, 2, 0), (4, 4, 1, 1, 0)])
@pytest.mark.parametrize("batch", [1, 3])
def test_conv2d_transpose_table_inverts_the_forward_table(hip, batch, h, w, k, stride, pad):
    fwd, ho, wo = ops.rulebook_conv2d(batch, h, w, k, k, stride, pad, "cuda")
    fwd = fwd.cpu().numpy()
    ref_fwd, rho, rwo = R.conv2d_table(batch, h, w, k, k, stride, pad)
    assert (ho, wo) == (rho, rwo) and np.array_equal(fwd, ref_fwd)
    n_in = batch * h * w
    out = Flat((k * k, n_in), n_in, dtype=torch.int32)
    rc = lib().cpd_rulebook_conv2d_transpose(batch, h, w, k, k, stride, pad, vp(out.view), stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = out.check(("conv2d transpose", batch, h, w, k, stride, pad), np.int32)
    assert np.array_equal(got, R.transpose_table(fwd, n_in))
    assert np.array_equal(T.rulebook_conv2d_transpose(batch, h, w, k, k, stride, pad, "cuda").cpu().numpy(), got)


def face_sites(rng, batch, shape, n):
    """about n sites of a [z, y, x] grid per batch, with sites on every face, edge and corner"""
    out = []
    for b in range(batch):
        cells = np.array([[z, y, x] for z in (0, shape[0] - 1) for y in (0, shape[1] // 2, shape[1] - 1) for x in (0, shape[2] // 2, shape[2] - 1)] +
                         [[shape[0] // 2, y, x] for y in (0, shape[1] - 1) for x in (0, shape[2] - 1)])
        lin = set((cells[:, 0] * shape[1] + cells[:, 1]) * shape[2] + cells[:, 2])
        lin |= set(rng.choice(shape[0] * shape[1] * shape[2], size=n - len(lin), replace=False).tolist())
        lin = np.array(sorted(lin))
        z, r = np.divmod(lin, shape[1] * shape[2])
        y, x = np.divmod(r, shape[2])
        out.append(np.stack([np.full_like(z, b), z, y, x], 1))
    return np.concatenate(out).astype(np.int32)


@gpu
@pytest.mark.parametrize("ksize,stride,pad", [([3, 3, 3], [2, 2, 2], [1, 1, 1]), ([3, 3, 3], [2, 2, 2], [0, 1, 1]), ([3, 1, 1], [2, 1, 1], [0, 0, 0])])
def test_conv_transpose_table_inverts_the_forward_table(hip, ksize, stride, pad):
    rng = np.random.default_rng(17)
    batch, shape = 2, [5, 9, 11]
    idx = face_sites(rng, batch, shape, 150)
    n_in, kv = idx.shape[0], ksize[0] * ksize[1] * ksize[2]
    assert 250 <= n_in <= 300
    for axis, size in enumerate(shape):
        assert (idx[:, axis + 1] == 0).any() and (idx[:, axis + 1] == size - 1).any()
    d_idx = torch.from_numpy(idx).cuda()
    out_idx, out_index, _ = ops.conv_outset(d_idx, batch, shape, ksize, stride, pad)
    index = ops.SiteIndex.build(d_idx, batch, shape)
    fwd = ops.rulebook_conv(out_idx, index, ksize, stride, pad).cpu().numpy()
    assert fwd.shape == (kv, out_idx.shape[0])

    def transposed(label):
        out = Flat((kv, n_in), n_in, dtype=torch.int32)
        rc = lib().cpd_rulebook_conv_transpose(vp(d_idx), n_in, batch, iarr(shape), iarr(ksize), iarr(stride), iarr(pad), vp(out_index.buf), vp(out.view),
                                               stream())
        assert rc == 0
        torch.cuda.synchronize()
        got = out.check(label, np.int32)
        assert np.array_equal(T.rulebook_conv_transpose(d_idx, batch, shape, ksize, stride, pad, out_index).cpu().numpy(), got)
        return got

    got = transposed("canonical order")
    assert np.array_equal(got, R.transpose_table(fwd, n_in))
    assert (got >= 0).sum() == (fwd >= 0).sum() > 0
    # once more over an output level whose rows were re-ordered after its index was built: the table names the NEW rows
    new_idx, n2o, o2n = ops.order_rows_by_taps(out_idx, out_index, chunk_rows=1024)
    out_index.set_order(o2n)
    fwd_p = ops.rulebook_conv(new_idx, index, ksize, stride, pad).cpu().numpy()
    assert np.array_equal(fwd_p, fwd[:, n2o.cpu().numpy()])
    got_p = transposed("tap-pattern order")
    out_index.set_order(None)
    assert np.array_equal(got_p, R.transpose_table(fwd_p, n_in))
