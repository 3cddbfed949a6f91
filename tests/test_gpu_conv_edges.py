"""ops.gather_conv at tile edges, odd row pitches and awkward tables, on every kernel family behind it.

Every case runs ONE small launch of a family forced through the planner's speed-only knobs (CPD_TUNE=1), asserts from the launch log
that the instantiation it meant to run is the one that ran, and compares with a float64 numpy restatement of

    out[j] = act((sum_t x[nbr[t, j]] . W[t]) * scale + shift + residual[j])

to the sparse tests' bound (1e-4 absolute). Input, output and residual are views into wider, taller buffers:
  * input padding columns and the rows from n_in to the end of the buffer hold NaN -- an over-read that reaches an accumulator
    turns the (finite) result into NaN;
  * the output buffer holds a fixed bit pattern with a full row tile of guard rows below n_out -- everything outside the rows
    and columns the call owns must come back bit-identical;
  * a row whose taps are all -1 must be relu(shift + residual) to the bit (0 * scale + shift is exact).
"""
import re
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from cpd_amd import ops

gpu = pytest.mark.gpu

PATTERN = 0x5A5A5A5A                 # what the output buffer holds before a call (a finite float: 1.5e16)
GUARD = 256                          # guard rows below n_out: the tallest row tile of any family
ATOL = 1e-4                          # the sparse tests' bound for these inputs (tests/test_gpu_sparse.py), against float64
PITCH = {"tight": (0, 0), "wide32": (32, 32), "pad4": (4, 4), "odd": (3, 1)}      # (pitch - c, column offset of the view)
EPILOGUES = {"none": (0, 0, 0, 0), "shift": (0, 1, 0, 0), "scale_shift": (1, 1, 0, 0), "residual": (0, 0, 1, 0), "relu": (0, 0, 0, 1),
             "all": (1, 1, 1, 1), "all_but_relu": (1, 1, 1, 0)}   # (scale, shift, residual, relu)
# (ReLU turns a NaN into 0 -- v > 0 ? v : 0 --, so the sweeps that look for over-reads also run without it: there a NaN that
# reached an accumulator arrives in the output, and the finiteness check names it)
KNOBS = ["CPD_GC_ROWWAVE_MIN", "CPD_GC_ROWWAVE_FLOOR", "CPD_GC_ROWWAVE_64", "CPD_GC_ROWWAVE_BN", "CPD_GC_RW8", "CPD_GC_RW8_MIN", "CPD_GC_BF16_MIN",
         "CPD_GC_BF16_MIN64", "CPD_GC_BF16_BN", "CPD_GC_WG", "CPD_GC_BM", "CPD_GC_BN", "CPD_GC_MS", "CPD_GC_NT", "CPD_GC_SPLIT", "CPD_GC_SPLIT_TILE",
         "CPD_GC_SPLIT_STAGES", "CPD_GC_RW_EPI", "CPD_GC_H16_EPI", "CPD_GC_PLANNED", "CPD_GC_PLANNED_MIN", "CPD_GC_BF16X3", "CPD_GC_DENSE_ROWWAVE",
         "CPD_GC_TAPS_INNER", "CPD_GC_BF16_DB", "CPD_GC_PLANNED_TB32"]
# what a launch falls back to when the planner's split / tile paths refuse a misaligned input (CPD_GC_MS / CPD_GC_NT below)
WAVE_FALLBACK = "gather_conv_kernel<2,1,false>"
RW_TAPS = 28                         # CPD_RW_TAPS: the most taps a row-wave launch takes


# ------------------------------------------------------------------------------------------------ reference (float64, logical arrays)
def conv_ref(x, w, nbr, scale=None, shift=None, residual=None, relu=False, n_out=None):
    """x [n_in, c_in], w [kv, c_in, c_out], nbr [kv, n_out] (or None: kv = 1, output row j < n_out reads row j) -> [n_out, c_out]
    float64. -1 entries contribute nothing."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    kv, n_out = (1, n_out) if nbr is None else nbr.shape
    if nbr is None:
        acc = x[:n_out] @ w[0]
    else:
        acc = np.zeros((n_out, w.shape[2]))
        for t in range(kv):
            hit = nbr[t] >= 0
            acc[hit] += x[nbr[t][hit]] @ w[t]
    if scale is not None:
        acc = acc * np.asarray(scale, np.float64)
    if shift is not None:
        acc = acc + np.asarray(shift, np.float64)
    if residual is not None:
        acc = acc + np.asarray(residual, np.float64)
    return np.maximum(acc, 0.0) if relu else acc


def scatter_ref(ref, buf_rows, width, off, row_map=None, col_group=0):
    """Where the launch must write: (values [buf_rows, width] float64, written mask). Row map and column-group scatter applied
    AFTER the arithmetic; everything the mask leaves out must keep the pattern."""
    n_out, c_out = ref.shape
    want = np.zeros((buf_rows, width))
    mask = np.zeros((buf_rows, width), bool)
    if col_group:
        for g in range(c_out // col_group):
            want[row_map[g], off:off + col_group] = ref[:, g * col_group:(g + 1) * col_group]
            mask[row_map[g], off:off + col_group] = True
    else:
        rows = np.arange(n_out) if row_map is None else row_map
        want[rows, off:off + c_out] = ref
        mask[rows, off:off + c_out] = True
    return want, mask


def pair_round(v):
    """fp32 value -> the fp32 value an fp16-pair row holds for it (h + l)"""
    v = np.asarray(v, np.float32)
    h = v.astype(np.float16)
    l = (v - h.astype(np.float32)).astype(np.float16)
    return h.astype(np.float32) + l.astype(np.float32)


def test_reference_agrees_with_the_oracle(oracle):
    """conv_ref against oracle.sparse_conv / oracle.affine_rows on a small SubM problem, to 1e-6. The inputs are dyadic rationals
    (multiples of 1/8 and 1/16 with small numerators), so the oracle's fp32 sums are exact and any difference is a mistake in one
    of the two restatements, not rounding."""
    rng = np.random.default_rng(3)
    batch, shape, cin, cout = 2, [4, 9, 11], 6, 10
    cells = rng.choice(batch * shape[0] * shape[1] * shape[2], size=300, replace=False)
    b, r = np.divmod(cells, shape[0] * shape[1] * shape[2])
    z, r = np.divmod(r, shape[1] * shape[2])
    y, x = np.divmod(r, shape[2])
    idx = np.stack([b, z, y, x], 1).astype(np.int32)
    nbr = oracle.subm_rulebook(idx, batch, shape, [3, 3, 3])
    assert (nbr < 0).any() and (nbr >= 0).sum() > 27 * 30
    feat = (rng.integers(-16, 17, size=(300, cin)) / 8.0).astype(np.float32)
    w = (rng.integers(-8, 9, size=(cout, 3, 3, 3, cin)) / 16.0).astype(np.float32)
    scale = rng.choice([0.5, 1.0, 1.5], cout).astype(np.float32)
    shift = (rng.integers(-8, 9, cout) / 8.0).astype(np.float32)
    res = (rng.integers(-16, 17, size=(300, cout)) / 8.0).astype(np.float32)
    w_kio = w.reshape(cout, 27, cin).transpose(1, 2, 0)
    np.testing.assert_allclose(conv_ref(feat, w_kio, nbr, None, shift), oracle.sparse_conv(feat, w, shift, nbr), atol=1e-6, rtol=0)
    for relu in (False, True):
        want = oracle.affine_rows(oracle.sparse_conv(feat, w, None, nbr), scale, shift, res, relu)
        np.testing.assert_allclose(conv_ref(feat, w_kio, nbr, scale, shift, res, relu), want, atol=1e-6, rtol=0)
    np.testing.assert_allclose(conv_ref(feat[:, :cin], w_kio[13:14], None), feat.astype(np.float64) @ w_kio[13].astype(np.float64), atol=0, rtol=0)


# ------------------------------------------------------------------------------------------------ families
@dataclass(frozen=True)
class Fam:
    key: str
    kind: str              # wave | h16 | tile | tsplit | rw | wide | plan
    c_in: int
    c_out: int
    math: str
    T: int                 # rows per workgroup (wave kernel: per wave tile)
    name: str              # the instantiation; "%s": the vector flag (wave) / the LDS-epilogue suffix (rw)
    env: tuple = ()
    dense: bool = False
    pairs: bool = False    # fp16-pair rows in, out and residual
    scaled: bool = False   # an absmax block comes with the input (the f16s forms)
    epi: bool = False      # rw: the LDS epilogue is on (the e / se / pe instantiations when the operands allow)
    split: int = 1         # rw: parts CPD_GC_SPLIT forces; tsplit: parts CPD_GC_SPLIT_TILE forces on a 27-tap launch
    plan: int = 0          # rows per tile of the row plan
    rows: tuple = ()       # row counts of the row sweep when the knobs only reach the instantiation there
    n_axis: int = 0        # row count of the other sweeps (default T + 1)
    axes: bool = True      # takes part in the pitch / epilogue / table sweeps (else: rows only)

    def sweep(self):
        T = self.T
        return self.rows or (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 1)

    def n(self):
        return self.n_axis or self.T + 1

    def __str__(self):
        return self.key


def _families():
    f = []
    # fp32 wave kernel: (c_in, c_out) of the issue, tile shapes pinned through CPD_GC_MS / CPD_GC_NT
    for cin, cout, ms, nt in [(5, 16, 1, 1), (16, 16, 2, 1), (32, 64, 4, 2), (32, 11, 2, 1), (20, 24, 1, 2)]:
        f.append(Fam("wave_%d_%d" % (cin, cout), "wave", cin, cout, "f32", 16 * ms, "gather_conv_kernel<%d,%d,%%s>" % (ms, nt),
                     (("CPD_GC_MS", ms), ("CPD_GC_NT", nt))))
    # 16-channel pair rows (K = 16 MFMA), LDS epilogue on and off
    for cout, nt in [(16, 1), (32, 2)]:
        for e in (1, 0):
            f.append(Fam("h16_%d_epi%d" % (cout, e), "h16", 16, cout, "f16x2", 32, "gather_conv_h16_kernel<2,%d>" % nt,
                         (("CPD_GC_MS", 2), ("CPD_GC_NT", nt), ("CPD_GC_H16_EPI", e)), pairs=True))
    # fp32 workgroup tiles
    f.append(Fam("tile_64_64", "tile", 32, 64, "f32", 64, "tile_conv_kernel<64,64>", (("CPD_GC_WG", 1),)))
    f.append(Fam("tile_64_128", "tile", 32, 128, "f32", 64, "tile_conv_kernel<64,128>", (("CPD_GC_WG", 1), ("CPD_GC_BN", 128))))
    # split workgroup tiles (dense flag): 64- and 128-row tiles, stage split on and off
    big, small = (("CPD_GC_BF16_MIN", 1),), (("CPD_GC_BF16_MIN", 10 ** 9), ("CPD_GC_BF16_MIN64", 1))
    for fl, math, sc in [("bf16", "bf16x3", False), ("f16", "f16x2", False), ("f16s", "f16x2", True)]:
        f.append(Fam("t%s_128x64" % fl, "tsplit", 64, 64, math, 128, "tile_conv_%s_kernel<128,64>" % fl, big, dense=True, scaled=sc))
        f.append(Fam("t%s_64x128" % fl, "tsplit", 32, 128, math, 64, "tile_conv_%s_kernel<64,128>" % fl, small, dense=True, scaled=sc))
        f.append(Fam("t%s_128x128_split" % fl, "tsplit", 64, 128, math, 128, "tile_conv_%s_kernel<128,128>" % fl, big + (("CPD_GC_SPLIT_TILE", 2),),
                     dense=True, scaled=sc, split=2))
        f.append(Fam("t%s_64x64_split" % fl, "tsplit", 64, 64, math, 64, "tile_conv_%s_kernel<64,64>" % fl, small + (("CPD_GC_SPLIT_TILE", 2),),
                     dense=True, scaled=sc, split=2, axes=False))
    # row-wave kernels: column tiles 32 / 64 / 128, 128- and 64-row workgroups. The 64-row forms of the wider tiles exist where
    # 64-row tiling makes more workgroups than 128-row tiling does (n_out > 64) or where a narrower tile does (two column tiles)
    one, floor, two = (("CPD_GC_ROWWAVE_MIN", 1),), (("CPD_GC_ROWWAVE_MIN", 10 ** 9), ("CPD_GC_ROWWAVE_FLOOR", 1)), (("CPD_GC_ROWWAVE_MIN", 2),)
    shapes = [(32, 2, 32, 32, one, (), 0, False), (64, 2, 64, 64, one, (1, 17, 129, 257), 0, True), (128, 2, 32, 128, one, (1, 17, 129, 257), 0, False),
              (32, 1, 32, 32, floor, (), 0, True), (64, 1, 64, 128, two, (1, 17, 63, 64), 49, False), (128, 1, 32, 128, two, (65, 127, 128), 65, True)]
    for fl, math, sc, pr, epi in [("bf16", "bf16x3", False, False, False), ("f16", "f16x2", False, False, False), ("f16", "f16x2", False, False, True),
                                  ("f16s", "f16x2", True, False, False), ("f16s", "f16x2", True, False, True), ("f16p", "f16x2", False, True, False),
                                  ("f16p", "f16x2", False, True, True)]:
        for bn, ms, cin, cout, env, rows, n_axis, axes in shapes:
            env = env + (() if fl == "bf16" else (("CPD_GC_RW_EPI", int(epi)),))
            f.append(Fam("rw_%s%s_%dx%d" % (fl, "e" if epi else "", bn, ms), "rw", cin, cout, math, 64 * ms, "rowwave_conv_%s%%s_kernel<%d,%d>" % (fl, bn, ms),
                         env, pairs=pr, scaled=sc, epi=epi, rows=rows, n_axis=n_axis, axes=axes))
    # wide workgroups on pair rows (256 rows; 192 at 128 columns)
    wide = one + (("CPD_GC_RW8", 224), ("CPD_GC_RW8_MIN", 1))
    f.append(Fam("rw_f16pw_32", "wide", 32, 32, "f16x2", 256, "rowwave_conv_f16pw_kernel<32,8>", wide, pairs=True))
    f.append(Fam("rw_f16pw_64", "wide", 64, 64, "f16x2", 256, "rowwave_conv_f16pw_kernel<64,8>", wide, pairs=True, rows=(1, 17, 257), axes=False))
    f.append(Fam("rw_f16pw_128", "wide", 32, 128, "f16x2", 192, "rowwave_conv_f16pw_kernel<128,6>", wide, pairs=True))
    # tap split behind a row-wave kernel
    for parts in (2, 4):
        f.append(Fam("rw_f16_split%d" % parts, "rw", 32, 32, "f16x2", 64, "rowwave_conv_f16%s_kernel<32,1>", floor + (("CPD_GC_SPLIT", parts),), epi=True,
                     split=parts))
    f.append(Fam("rw_f16s_split2", "rw", 64, 64, "f16x2", 128, "rowwave_conv_f16s%s_kernel<64,2>", one + (("CPD_GC_SPLIT", 2),), scaled=True, epi=True, split=2))
    f.append(Fam("rw_f16p_split2", "rw", 32, 128, "f16x2", 128, "rowwave_conv_f16p%s_kernel<128,2>", one + (("CPD_GC_SPLIT", 2),), pairs=True, epi=True,
                 split=2))
    f.append(Fam("rw_bf16_split4", "rw", 32, 32, "bf16x3", 128, "rowwave_conv_bf16%s_kernel<32,2>", one + (("CPD_GC_SPLIT", 4),), split=4, axes=False))
    # staged row-wave kernel through a row plan
    for tile in (128, 256):
        for cin, cout in [(32, 32), (64, 64), (32, 128)]:
            f.append(Fam("plan%d_%d_%d" % (tile, cin, cout), "plan", cin, cout, "f16x2", tile, "rowplan_conv_f16p_kernel<%d%s>" % (cout, ",256" if tile == 256 else ""),
                         (("CPD_GC_PLANNED_MIN", 1),) + one, pairs=True, plan=tile, axes=cin != 64))
    return f


FAMILIES = _families()
AXES = [f for f in FAMILIES if f.axes]
# every family of the issue's table, as a pattern one logged name must match
REQUIRED = [r"gather_conv_kernel<\d,\d,true>", r"gather_conv_kernel<\d,\d,false>", r"gather_conv_h16_kernel<", r"tile_conv_kernel<64,64>",
            r"tile_conv_kernel<64,128>", r"tile_conv_bf16_kernel<64,", r"tile_conv_bf16_kernel<128,", r"tile_conv_f16_kernel<64,", r"tile_conv_f16_kernel<128,",
            r"tile_conv_f16s_kernel<64,", r"tile_conv_f16s_kernel<128,", r"rowwave_conv_f16pw_kernel<", r"split_finish_kernel",
            r"rowplan_conv_f16p_kernel<\d+>", r"rowplan_conv_f16p_kernel<\d+,256>"] + \
           [r"rowwave_conv_%s_kernel<%d,%d>" % (fl, bn, ms) for fl in ("bf16", "f16", "f16e", "f16s", "f16se", "f16p", "f16pe") for bn in (32, 64, 128)
            for ms in (1, 2)]
LOGGED = set()


def set_knobs(mp, fam):
    mp.setenv("CPD_TUNE", "1")                   # the knobs are only read when this is set
    for k in KNOBS:
        mp.delenv(k, raising=False)
    env = {"CPD_GC_SPLIT": 1, "CPD_GC_SPLIT_TILE": 0, "CPD_GC_MS": 2, "CPD_GC_NT": 1}
    env.update(dict(fam.env))
    for k, v in env.items():
        mp.setenv(k, str(v))


def aligned(c, pitch):
    pad, off = PITCH[pitch]
    return (c + pad) % 4 == 0 and off % 4 == 0


def expected(fam, kv, in_al, out_al, res_al, ss_al, mapped=False, grouped=False):
    """(conv instantiation, parts) the launcher must choose: gather_conv_impl's alignment switches, restated"""
    if fam.kind == "wave":
        return fam.name % ("true" if in_al and fam.c_in % 16 == 0 else "false"), 1
    if fam.kind in ("h16", "plan", "wide"):
        return fam.name, 1
    if not in_al:
        return WAVE_FALLBACK, 1                  # no 16-byte gathers: the fp32 wave kernel's element-wise form
    if fam.kind == "tile":
        return fam.name, 1
    vec_out = out_al and res_al and not grouped
    parts = fam.split if (fam.split > 1 and vec_out and ss_al) else 1
    if fam.kind == "tsplit":
        return fam.name, parts if kv * (fam.c_in // 32) >= 32 else 1
    e = "e" if (fam.epi and vec_out and parts == 1 and not mapped) else ""
    return fam.name % e, parts


_WEIGHTS = {}


def weights(c_in, c_out, kv):
    """[kv, c_in, c_out] weights and their packed image, once per shape"""
    key = (c_in, c_out, kv)
    if key not in _WEIGHTS:
        rng = np.random.default_rng(c_in * 100003 + c_out * 101 + kv)
        w = (rng.normal(size=(kv, c_in, c_out)) * np.sqrt(2.0 / (kv * c_in))).astype(np.float32)
        _WEIGHTS[key] = (w, ops.pack_weight(torch.from_numpy(w).cuda()))
    return _WEIGHTS[key]


def make_table(rng, kind, kv, n_in, n_out, T):
    """host-built tables (no tap masks): about half the entries -1, then the shape under test"""
    nbr = rng.integers(0, n_in, size=(kv, n_out)).astype(np.int32)
    nbr[rng.random((kv, n_out)) < 0.5] = -1
    if kind == "tap_off":
        nbr[kv // 2] = -1
    elif kind == "row_off":
        nbr[:, n_out // 2] = -1
        nbr[:, n_out - 1] = -1
    elif kind == "last_tile":
        nbr[:, ((n_out - 1) // T) * T:] = n_in - 1
    elif kind == "one_row":
        nbr[:] = n_in // 2
    else:
        assert kind == "rand"
    return nbr


def in_buffer(rows, pitch, extra=3):
    """rows [n, c] (device) as a view of a NaN-filled buffer with `extra` more rows"""
    pad, off = PITCH[pitch]
    n, c = rows.shape
    buf = torch.full((n + extra, c + pad), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:n, off:off + c]
    view.copy_(rows)
    return view


def launch(fam, mp, label, *, n_in, n_out, kv, nbr=None, nbr_dev=None, pitches=("tight", "tight", "tight"), epi="all", ss_offset=False,
           mapped=False, grouped=False, seed=0):
    """One launch of `fam` with every check of this file; -> (logical result [n_out, c_out] fp32 numpy, logged counts).
    nbr: host table (or None with kv = 1); nbr_dev: a device table that carries its own attributes (tap masks)."""
    set_knobs(mp, fam)
    rng = np.random.default_rng(seed + 7919 * n_out + kv)
    c_in, c_out = fam.c_in, fam.c_out
    p_in, p_out, p_res = pitches
    use_scale, use_shift, use_res, relu = EPILOGUES[epi]
    w, packed = weights(c_in, c_out, kv)
    x = torch.from_numpy(rng.normal(size=(n_in, c_in)).astype(np.float32)).cuda()
    res = torch.from_numpy(rng.normal(size=(n_out, c_out)).astype(np.float32)).cuda() if use_res else None
    xs, rs = x, res
    if fam.pairs:                                # the reference input is what the pair rows hold
        xs = ops.rows_to_pairs(x)
        x = ops.pairs_to_rows(xs)
        if use_res:
            rs = ops.rows_to_pairs(res)
            res = ops.pairs_to_rows(rs)
    x_view = in_buffer(xs, p_in)
    r_view = in_buffer(rs, p_res) if use_res else None
    ss = torch.empty((2, c_out + 4), dtype=torch.float32, device="cuda")
    o = 1 if ss_offset else 0                    # views 4 bytes into their buffers: not 16-byte aligned
    scale = shift = None
    if use_scale:
        scale = ss[0, o:o + c_out]
        scale.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c_out).astype(np.float32)))
    if use_shift:
        shift = ss[1, o:o + c_out]
        shift.copy_(torch.from_numpy(rng.normal(size=c_out).astype(np.float32)))
    # output buffer: the pattern everywhere, a row tile of guard rows below the rows the call may write
    pad, off = PITCH[p_out]
    groups = 4 if grouped else 1
    width = (c_out // groups) + pad
    buf_rows = groups * n_out + GUARD
    row_map = None
    if mapped or grouped:
        row_map = rng.permutation(buf_rows)[:groups * n_out].astype(np.int32).reshape(groups, n_out)
    out_i = torch.full((buf_rows, width), PATTERN, dtype=torch.int32, device="cuda")
    out_view = out_i.view(torch.float32)[:(buf_rows if row_map is not None else n_out), off:off + c_out // groups]
    if nbr_dev is None and nbr is not None:
        nbr_dev = torch.from_numpy(nbr).cuda()
    if nbr_dev is not None and nbr is None:
        nbr = nbr_dev.cpu().numpy()
    if nbr is not None:
        assert nbr.shape == (kv, n_out) and nbr.min() >= -1 and nbr.max() < n_in      # never an out-of-range index
    else:
        assert kv == 1 and n_in >= n_out
    if fam.plan:
        ops.rulebook_plan(nbr_dev, fam.plan)
    block = ops.absmax_blocks(1, "cuda")[0]
    kw = dict(math=fam.math, dense=fam.dense, out=out_view, out_absmax=block)
    if fam.pairs:
        kw.update(in_pairs=True, out_pairs=True, res_pairs=use_res)
    if fam.scaled:
        kw["in_absmax"] = ops.absmax_rows(x_view, c_in)
    if row_map is not None:
        kw["out_row_map"] = torch.from_numpy(row_map).cuda().reshape(-1).contiguous()
        kw["out_col_group"] = c_out // 4 if grouped else 0
    with ops.launch_log() as log:
        ops.gather_conv(x_view, c_in, packed, nbr_dev, kv, n_out, c_out, scale, shift, r_view, bool(relu), **kw)
    torch.cuda.synchronize()
    LOGGED.update(log.counts)

    # ---- which kernel ran
    in_al, out_al = aligned(c_in, p_in), aligned(c_out // groups, p_out)
    res_al = aligned(c_out, p_res) or not use_res
    ss_al = not (ss_offset and (use_scale or use_shift))
    name, parts = expected(fam, kv, in_al, out_al, res_al, ss_al, mapped, grouped)
    want_log = {name: 1}
    if parts > 1:
        want_log["split_finish_kernel"] = 1
    assert log.counts == want_log, (label, log.counts, want_log)
    if in_al:                                    # (the planner query has no pointer to look at: aligned inputs only)
        told = ops.gather_conv_tile(n_out, c_in, c_out, x_view.stride(0), dense=fam.dense, nbr=nbr_dev, math=fam.math, scaled=fam.scaled,
                                    in_pairs=fam.pairs, kv=kv)
        strip = lambda s: re.sub(r"_(f16s?p?)e_kernel", r"_\1_kernel", s)
        assert strip(told) == strip(name), (label, told, name)

    # ---- what it wrote, and what it left alone
    got_i = out_i.cpu().numpy()
    ref = conv_ref(x.cpu().numpy(), w, nbr, scale.cpu().numpy() if use_scale else None, shift.cpu().numpy() if use_shift else None,
                   res.cpu().numpy() if use_res else None, relu, n_out)
    assert np.isfinite(ref).all() and ref.shape == (n_out, c_out)
    want, mask = scatter_ref(ref, buf_rows, width, off, None if row_map is None else (row_map if grouped else row_map[0]), c_out // 4 if grouped else 0)
    stray = np.argwhere((got_i != PATTERN) & ~mask)
    assert stray.size == 0, (label, "wrote outside its rows / columns at (row, column)", stray[:8].tolist(), "n_out", n_out, "off", off)
    if fam.pairs:
        rows = torch.from_numpy(np.arange(n_out) if row_map is None else row_map[0].astype(np.int64)).cuda()
        got = ops.pairs_to_rows(out_i.view(torch.float32)[rows][:, off:off + c_out].contiguous()).cpu().numpy()
    elif grouped:
        got_f = got_i.view(np.float32)
        got = np.concatenate([got_f[row_map[g], off:off + c_out // 4] for g in range(4)], 1)
    else:
        got = got_i.view(np.float32)[np.arange(n_out) if row_map is None else row_map[0], off:off + c_out]
    assert np.isfinite(got).all(), (label, "NaN / inf in the result: a padding column or a row past n_in reached an accumulator",
                                    np.argwhere(~np.isfinite(got))[:8].tolist())
    np.testing.assert_allclose(got, ref, atol=ATOL, rtol=0, err_msg=str(label))
    if nbr is not None:
        dead = (nbr < 0).all(0)
        if dead.any():                           # no neighbour at all: relu(shift + residual), to the bit
            e = np.zeros((int(dead.sum()), c_out), np.float32)
            if use_shift:
                e = e + shift.cpu().numpy()
            if use_res:
                e = e + res.cpu().numpy()[dead]
            if relu:
                e = np.where(e > 0, e, np.float32(0))
            e = pair_round(e) if fam.pairs else e
            assert np.array_equal(got[dead].view(np.int32), e.astype(np.float32).view(np.int32)), (label, "rows without neighbours", np.flatnonzero(dead)[:8])
    # ---- the absmax block: exactly max |out| (pair rows hold the rounded value of what the epilogue measured)
    am, top = np.float32(ops.absmax_value(block)), np.float32(np.abs(got).max())
    assert top == am or (fam.pairs and top == pair_round(am)), (label, "out_absmax", float(am), float(top))
    return got, log.counts


def n_in_for(fam, n_out):
    sweep = fam.sweep()
    return 300 if n_out == 1 else (7 if n_out == max(sweep) else 50)


# ------------------------------------------------------------------------------------------------ axis 1: rows
@gpu
@pytest.mark.parametrize("fam,n_out", [pytest.param(f, n, id="%s-n%d" % (f.key, n)) for f in FAMILIES for n in f.sweep()])
def test_row_counts_around_the_tile(hip, monkeypatch, fam, n_out):
    """n_out at 1, around the 16-row sub-tile and around the workgroup's row tile; n_in chosen apart from n_out (7 rows behind the
    largest launch, 300 behind a single output row); tables with a dead row in the middle and at the tail, and with every row of
    the last tile on input row n_in - 1."""
    n_in = n_in_for(fam, n_out)
    rng = np.random.default_rng(n_out)
    for kind, epi in (("rand", "all_but_relu"), ("row_off", "all"), ("last_tile", "all")):
        nbr = make_table(rng, kind, 27, n_in, n_out, fam.T)
        launch(fam, monkeypatch, (fam.key, "n_out", n_out, "n_in", n_in, kind, epi), n_in=n_in, n_out=n_out, kv=27, nbr=nbr, epi=epi)


# ------------------------------------------------------------------------------------------------ axis 2: tables
@gpu
@pytest.mark.parametrize("fam,kv", [pytest.param(f, kv, id="%s-kv%d" % (f.key, kv)) for f in AXES for kv in (1, 4, 9, 27, 32)
                                    if f.kind != "plan" or kv == 27])           # (the row plan is a 27-tap plan)
def test_table_shapes(hip, monkeypatch, fam, kv):
    """kv = 1 without a table, 4, 9, 27 and 32 taps (the row-wave kernels keep 28: a 32-tap launch must go elsewhere, or be refused
    on pair rows); random tables, a whole tap off, whole rows off, the last tile on input row n_in - 1, every row on one input row."""
    n_out = fam.n()
    if kv > RW_TAPS and fam.kind in ("rw", "wide"):
        # more taps than a row-wave launch keeps: fp32 rows go to the wave kernel, pair rows (which nothing else reads) are refused
        set_knobs(monkeypatch, fam)
        nbr = make_table(np.random.default_rng(kv), "rand", kv, 50, n_out, fam.T)
        if fam.pairs:
            x = ops.rows_to_pairs(torch.zeros((50, fam.c_in), device="cuda"))
            with pytest.raises(ops._lib.CpdHipError):
                ops.gather_conv(x, fam.c_in, weights(fam.c_in, fam.c_out, kv)[1], torch.from_numpy(nbr).cuda(), kv, n_out, fam.c_out, math=fam.math,
                                in_pairs=True, out_pairs=True)
            return
        wave = Fam(fam.key + "_kv32", "wave", fam.c_in, fam.c_out, fam.math, 32, "gather_conv_kernel<2,1,%s>", fam.env, scaled=fam.scaled)
        launch(wave, monkeypatch, (fam.key, "kv", kv), n_in=50, n_out=n_out, kv=kv, nbr=nbr)
        return
    if kv == 1:
        launch(fam, monkeypatch, (fam.key, "kv 1, no table"), n_in=n_out + 5, n_out=n_out, kv=1, nbr=None)
        return
    rng = np.random.default_rng(kv)
    for kind in ("rand", "tap_off", "row_off", "last_tile", "one_row"):
        for n_in in (7, 50):
            nbr = make_table(rng, kind, kv, n_in, n_out, fam.T)
            launch(fam, monkeypatch, (fam.key, "kv", kv, kind, "n_in", n_in), n_in=n_in, n_out=n_out, kv=kv, nbr=nbr)


@gpu
@pytest.mark.parametrize("fam", AXES, ids=str)
def test_device_built_subm_table_with_and_without_tap_masks(hip, monkeypatch, fam):
    """ops.SiteIndex.build + ops.rulebook_subm on a site set of exactly n_out sites, with its tap masks -- and the same table
    without them: a skipped (sub-tile, tap) pair adds exact zeros, so an unsplit launch gives the same bits either way."""
    n = fam.n()
    rng = np.random.default_rng(n)
    shape = [5, 14, 14]
    cells = np.sort(rng.choice(shape[0] * shape[1] * shape[2], size=n, replace=False))
    z, r = np.divmod(cells, shape[1] * shape[2])
    y, x = np.divmod(r, shape[2])
    idx = torch.from_numpy(np.stack([np.zeros_like(z), z, y, x], 1).astype(np.int32)).cuda()
    nbr = ops.rulebook_subm(idx, ops.SiteIndex.build(idx, 1, shape))
    assert nbr.shape == (27, n) and nbr.tapmask is not None
    masked, counts = launch(fam, monkeypatch, (fam.key, "subm, masks"), n_in=n, n_out=n, kv=27, nbr_dev=nbr, seed=5)
    plain, _ = launch(fam, monkeypatch, (fam.key, "subm, no masks"), n_in=n, n_out=n, kv=27, nbr_dev=nbr.clone(), seed=5)
    if "split_finish_kernel" not in counts:      # (a tap split deals the ACTIVE taps: the parts differ with the masks)
        assert np.array_equal(masked.view(np.int32), plain.view(np.int32)), fam.key


# ------------------------------------------------------------------------------------------------ axis 3: pitch and alignment
def _pitch_cases(fam):
    kinds = ("wide32", "pad4") if fam.pairs else ("wide32", "pad4", "odd")     # pair rows: aligned offsets only
    out = []
    for k in kinds:
        out += [("in_" + k, (k, "tight", "tight")), ("out_" + k, ("tight", k, "tight")), ("res_" + k, ("tight", "tight", k)), ("all_" + k, (k, k, k))]
    return out


@gpu
@pytest.mark.parametrize("fam,case,pitches", [pytest.param(f, c, p, id="%s-%s" % (f.key, c)) for f in AXES for c, p in _pitch_cases(f)])
def test_pitch_and_alignment(hip, monkeypatch, fam, case, pitches):
    """input / output / residual as views [rows, off : off + c] of wider buffers, each alone and all together; the launch log must
    show the epilogue or gather form the alignment selects (asserted in launch(): f16e -> f16, no split, the element-wise wave kernel)."""
    n_out = fam.n()
    nbr = make_table(np.random.default_rng(len(case)), "row_off", 27, 50, n_out, fam.T)
    launch(fam, monkeypatch, (fam.key, case, "no ReLU"), n_in=50, n_out=n_out, kv=27, nbr=nbr, pitches=pitches, epi="all_but_relu")
    _, counts = launch(fam, monkeypatch, (fam.key, case), n_in=50, n_out=n_out, kv=27, nbr=nbr, pitches=pitches)
    if "odd" in case and fam.kind in ("rw", "tsplit"):
        assert "split_finish_kernel" not in counts and not any(re.search(r"_f16s?p?e_kernel", k) for k in counts), (fam.key, case, counts)
        if case.startswith(("in_", "all_")):
            assert list(counts) == [WAVE_FALLBACK], (fam.key, case, counts)


@gpu
@pytest.mark.parametrize("fam", AXES, ids=str)
def test_scale_and_shift_at_a_four_byte_offset(hip, monkeypatch, fam):
    n_out = fam.n()
    nbr = make_table(np.random.default_rng(1), "rand", 27, 50, n_out, fam.T)
    _, counts = launch(fam, monkeypatch, (fam.key, "scale / shift offset"), n_in=50, n_out=n_out, kv=27, nbr=nbr, ss_offset=True)
    assert "split_finish_kernel" not in counts, (fam.key, counts)         # the finish kernel reads them as 16-byte pieces


@gpu
def test_pair_rows_at_a_misaligned_offset_are_refused(hip, monkeypatch):
    """fp16-pair input needs whole 16-byte pieces: a view one float into its buffer (pitch c + 3) is refused, and nothing runs"""
    for key in ("rw_f16pe_32x1", "h16_16_epi1", "rw_f16pw_32"):
        fam = next(f for f in FAMILIES if f.key == key)
        set_knobs(monkeypatch, fam)
        x = in_buffer(ops.rows_to_pairs(torch.ones((50, fam.c_in), device="cuda")), "odd")
        nbr = torch.from_numpy(make_table(np.random.default_rng(2), "rand", 27, 50, 65, fam.T)).cuda()
        out_i = torch.full((65 + GUARD, fam.c_out), PATTERN, dtype=torch.int32, device="cuda")
        with ops.launch_log() as log:
            with pytest.raises(ops._lib.CpdHipError):
                ops.gather_conv(x, fam.c_in, weights(fam.c_in, fam.c_out, 27)[1], nbr, 27, 65, fam.c_out, math="f16x2", in_pairs=True, out_pairs=True,
                                out=out_i.view(torch.float32)[:65])
        torch.cuda.synchronize()
        assert log.counts == {} and bool((out_i == PATTERN).all()), (key, log.counts)


# ------------------------------------------------------------------------------------------------ epilogues
@gpu
@pytest.mark.parametrize("epi", ["none", "shift", "scale_shift", "residual", "relu", "all"])
@pytest.mark.parametrize("fam", AXES, ids=str)
def test_epilogues(hip, monkeypatch, fam, epi):
    n_out = fam.n()
    nbr = make_table(np.random.default_rng(len(epi)), "row_off", 27, 50, n_out, fam.T)
    launch(fam, monkeypatch, (fam.key, epi), n_in=50, n_out=n_out, kv=27, nbr=nbr, epi=epi)


@gpu
@pytest.mark.parametrize("fam", [f for f in AXES if f.kind != "plan"], ids=str)
def test_out_row_map_leaves_unnamed_rows_alone(hip, monkeypatch, fam):
    """an injective row map into a taller buffer: the rows it does not name keep the pattern (the whole buffer is compared)"""
    n_out = fam.n()
    nbr = make_table(np.random.default_rng(3), "row_off", 27, 50, n_out, fam.T)
    launch(fam, monkeypatch, (fam.key, "row map"), n_in=50, n_out=n_out, kv=27, nbr=nbr, mapped=True)
    launch(fam, monkeypatch, (fam.key, "row map, wide32"), n_in=50, n_out=n_out, kv=27, nbr=nbr, mapped=True, pitches=("tight", "wide32", "tight"))


@gpu
@pytest.mark.parametrize("fam", [f for f in AXES if not f.pairs and f.c_out % 4 == 0 and f.kind != "plan"], ids=str)
def test_column_group_scatter(hip, monkeypatch, fam):
    """out_col_group = c_out / 4: column group g of output row j lands in row map[g][j], columns [0, c_out / 4) of the view"""
    n_out = fam.n()
    nbr = make_table(np.random.default_rng(4), "row_off", 27, 50, n_out, fam.T)
    for p_out in ("tight", "wide32", "odd"):
        launch(fam, monkeypatch, (fam.key, "column groups", p_out), n_in=50, n_out=n_out, kv=27, nbr=nbr, grouped=True, pitches=("tight", p_out, "tight"))


# ------------------------------------------------------------------------------------------------ coverage
@gpu
def test_every_family_of_the_table_is_reached(hip, monkeypatch):
    """one launch per family spec; every kernel family behind ops.gather_conv appears in a logged name"""
    seen = set()
    for fam in FAMILIES:
        n_out = fam.sweep()[-1]
        nbr = make_table(np.random.default_rng(9), "rand", 27, 50, n_out, fam.T)
        _, counts = launch(fam, monkeypatch, (fam.key, "coverage"), n_in=50, n_out=n_out, kv=27, nbr=nbr)
        seen.update(counts)
    # the forms only a misaligned operand selects
    for key, pitches in (("wave_16_16", ("odd", "tight", "tight")), ("rw_f16e_32x1", ("tight", "odd", "tight"))):
        fam = next(f for f in FAMILIES if f.key == key)
        nbr = make_table(np.random.default_rng(9), "rand", 27, 50, fam.n(), fam.T)
        seen.update(launch(fam, monkeypatch, (key, "coverage", pitches), n_in=50, n_out=fam.n(), kv=27, nbr=nbr, pitches=pitches)[1])
    missing = [pat for pat in REQUIRED if not any(re.match(pat, s) for s in seen)]
    print("instantiations logged:", *sorted(seen), sep="\n  ")
    assert not missing, missing
