"""Fused forward engine of the hot path: points -> boxes, one process per GPU.

Mirrors CenterPoint.forward's module_topology (cpd/models/detectors/detector3d_template.py:22-25,
centerpoint.py:9-22) for the one-stage path
    MeanVFE -> VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone -> CenterHead -> NMS
but as a flat list of C-ABI launches on one HIP stream: eval-mode BatchNorm, bias, ReLU and the
SparseBasicBlock residual are folded into the conv epilogues, activations stay channels-last in
HBM, rulebooks are built once per indice_key, and nothing leaves the device until the final boxes.
Weights come in under the reference's own state_dict names (so a CPD checkpoint loads unchanged).
"""
import contextlib
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional

import torch

from . import _lib, layer_table, ops, train_ops
from .layer_table import _DOWN, STRIDED_STAGES, final_shape      # noqa: F401  (_DOWN: importable from here as before)
from .range_guard import GUARDED_BITS, OPTIMISTIC_BITS, BlockPool, RangeGuard


@dataclass
class ModelConfig:
    """The fields of voxel_rcnn_cproto_center.yaml / waymo_unsupervised_cproto.yaml the path reads."""
    point_cloud_range: List[float] = field(default_factory=lambda: [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0])
    voxel_size: List[float] = field(default_factory=lambda: [0.1, 0.1, 0.15])
    max_points_per_voxel: int = 5
    max_voxels: int = 1000000
    num_point_features: int = 5
    num_filters: List[int] = field(default_factory=lambda: [16, 32, 64, 128])      # BACKBONE_3D.NUM_FILTERS
    out_features: int = 128                                                        # BACKBONE_3D.OUT_FEATURES
    bev_layer_nums: List[int] = field(default_factory=lambda: [5, 5])              # BACKBONE_2D.*
    bev_layer_strides: List[int] = field(default_factory=lambda: [1, 2])
    bev_num_filters: List[int] = field(default_factory=lambda: [128, 256])
    bev_upsample_strides: List[int] = field(default_factory=lambda: [1, 2])
    bev_num_upsample_filters: List[int] = field(default_factory=lambda: [256, 256])
    shared_conv_channel: int = 64                                                  # DENSE_HEAD.*
    num_class: int = 3
    head_order: List[str] = field(default_factory=lambda: ["center", "center_z", "dim", "rot"])
    head_channels: Dict[str, int] = field(default_factory=lambda: {"center": 2, "center_z": 1, "dim": 3, "rot": 2})
    feature_map_stride: int = 8
    score_thresh: float = 0.1
    post_center_limit_range: List[float] = field(default_factory=lambda: [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0])
    max_obj_per_sample: int = 500
    nms_thresh: float = 0.8
    nms_pre_maxsize: int = 4096
    nms_post_maxsize: int = 500
    # arithmetic of the convolutions with >= 32 input channels (include/cpd_hip.h): "f16x2" = fp32 operands written as two fp16
    # terms, three partial products accumulated in fp32 on the 16-bit matrix pipe (fp32-level error; fp16's range is guarded per
    # layer, `range_guard` below: any activation magnitude gives the fp32 answer, CPD_GC_F16X2); "bf16x3" = three bf16 terms, six partial
    # products (exact split over the whole fp32 range, CPD_GC_BF16X3); "f32" = fp32-input MFMA everywhere (bitwise an fmaf chain)
    conv_math: str = "f16x2"
    # internal row order of the strided levels: "taps" = every chunk of `row_order_chunk` canonical rows sorted by neighbour
    # pattern, so that the conv kernels' 16-row tap skipping is nearly exact (ops.order_rows_by_taps; a level's exported
    # (features, indices) pair is in that order -- any order is a valid sparse tensor); "canonical" = ascending (b, z, y, x)
    # rows of level 0 inside the engine: "canonical" = ascending (frame, z, y, x), straight from the occupancy bitmap's ranks
    # (no first-appearance scan, canonical level-0 index, coherent lookups for the rulebooks built on it); "appearance" = the
    # voxelizer's boundary order (Point2VoxelCPU3d). Same voxels and features either way.
    # f16x2 only: every conv epilogue records the bits of max |output| and the next layer pre-scales its input by a power of
    # two taken from it (exact; the `*_f16s_*` kernels), so that an activation of ANY fp32 magnitude gives the fp32 answer where
    # unguarded split-fp16 arithmetic overflows to inf / NaN at 65504. False = the unscaled kernels.
    range_guard: bool = True
    voxel_row_order: str = "canonical"
    # storage of the activations BETWEEN the f16x2 sparse layers of levels 2-4 (engine-internal; every exported tensor is fp32):
    # True = fp16-pair rows (CPD_GC_*_PAIRS: the epilogue that produces a row writes its split x = h + l, the up to 27 gathers of
    # the row take the bits as MFMA fragments -- same products, no split in the stage loop); a range-guard re-run uses fp32 rows
    pair_rows: bool = True
    pair_rows_level1: bool = True          # ... and level 1 (16 channels: K = 16 MFMA form of the wave kernel) as well
    # ... and the DENSE half (round 5): conv_out writes pair rows, densify copies them, every BEV / head map between two split-fp16 layers
    # is a pair-row map (window_conv_f16p_kernel / tile_conv_f16p_kernel take the stored bits as MFMA fragments: no split in the
    # staging); the head's output maps are fp32. Only batches whose layers all take a window tile the pair kernels exist for (>= 2
    # frames at 188 x 188; engine.dense_pairs_ok): smaller batches keep fp32 dense maps. Exported tensors (bev_cat, encoded) are fp32.
    pair_rows_dense: bool = True
    persistent_dense_map: bool = True      # densify into a persistent pre-zeroed map, re-zero the occupied rows after its reader (ops.DenseMap)
    voxelizer_group: int = 64             # frames per batched-voxelizer call (its FrameOffsets kernel argument holds 64)
    batched_voxelizer_min_frames: int = 2  # smaller batches: one voxelizer call per frame + a separate level-0 index build
    # "bricks" (round 4, measured, NOT the default): rows of the strided levels in 8 x 8 (y, x) brick order of their z-plane,
    # pattern-sorted inside every 128-row tile (ops.order_rows_bricks); with plan_rulebooks their sub-manifold rulebooks are PLANNED
    # (ops.rulebook_plan) and the SparseBasicBlock convs of levels 2-4 run the staged row-wave kernel, which fetches a tile's distinct
    # input rows once into LDS instead of gathering every (row, tap) pair through the vector L1 (cpd_gather_conv_planned; needs
    # pair_rows). Same box, 48 frames: taps 1057, bricks 1045 (rulebooks -9 us/frame, row-wave kernels +5 %: coarser tap skipping),
    # bricks + plan 956 (the staged kernel moves half the bytes through the L1 but holds 8-12 waves per CU, not 25).
    row_order: str = "taps"
    row_order_brick: tuple = (8, 8)
    # "taps": level 0 (the voxel list) in tap-pattern order as well, when the voxelizer delivered canonical rows. Measured, same box, two
    # pairs: level-1 convs 51.8 -> 46.7 us/frame, rulebooks + the sort + the feature gather +6 us: 1046 vs 1049.5 frames/s -> off
    row_order_level0: bool = False
    chunked_rulebooks: bool = True         # "taps": rulebooks of the re-ordered levels built chunk-wise in canonical order (ops.rulebook_*(canonical=))
    plan_channels: tuple = (32, 64)        # levels (by channel count) whose SubM convs take the staged kernel when plan_rulebooks
    plan_tile_rows: int = 256              # rows per workgroup of the staged kernel / per pattern-sorted tile of the brick order (128 | 256)
    plan_rulebooks: bool = False           # "bricks" only: plan the sub-manifold rulebooks -> the staged row-wave kernel
    row_order_chunk: int = 4096
    row_order_min_rows: int = 65536        # below this a level does not fill the chip either way
    # the strided stages' index chain (output set, row order, rulebooks) on a second HIP stream, one stage ahead of the convolutions
    # (engine.backbone3d); batches above `index_side_stream_max_frames` fill the chip with every launch and keep one stream
    index_side_stream: bool = True
    # ... and the BEV deblocks that have a level of convolutions between them and the shared conv, for batches of up to
    # `deblock_side_stream_max_frames` frames (same box: one frame 2.84 -> 2.79 ms, 4 frames +0.6 %; at 48 frames the HBM-bound GEMM
    # slows the window convs it runs beside by more than it hides: 1240 -> 1227 frames/s)
    deblock_side_stream: bool = True
    deblock_side_stream_max_frames: int = 8
    index_side_stream_max_frames: int = 1 << 30
    # CenterHead's regression branches (center, center_z, dim, rot) only at the max_obj_per_sample merged top-K pixels of each frame -- the
    # only places the decode reads them (1.4 % of a 188 x 188 map): the hm branch alone runs over every pixel, the selection
    # (ops.center_peaks) names the winners, the regression branches' first convs run as ONE gather_conv over the 9 hidden sites around
    # each winner (ops.peak_rulebook) and ops.center_decode_at_peaks applies their last convs in fp32 and decodes. Scores, labels and
    # peak pixels are bit for bit those of the full maps (the hm branch takes the same kernel and tile as inside the fused layers: a batch
    # shape where it would not keeps the full maps, engine._head_at_peaks_ok); boxes differ by the last conv's fp32 summation order.
    # (Bit for bit on the unguarded kernels. In a range-guarded step head2_hm pre-scales its input by the power of two of the hm branch's
    # 64 hidden channels, the fused head2 by that of all 320: where the exponents differ the fp16 low terms round differently and a score
    # can differ in its last bits -- fp32-level, like everything else a guarded step changes.)
    # Callers that want the head maps (return_intermediates, bev_and_head on its own) get the full maps. CPD_HEAD_AT_PEAKS=0 in the
    # environment turns it off at construction (same-box A/B). Batches below head_at_peaks_min_frames keep the full maps
    # (the measured pairs).
    head_at_peaks: bool = True
    head_at_peaks_min_frames: int = 4

    @property
    def grid_zyx(self):
        return ops.voxel_grid_size(self.voxel_size, self.point_cloud_range)

    @property
    def sparse_shape(self):
        g = self.grid_zyx
        return [g[0] + 1, g[1], g[2]]     # grid_size[::-1] + [1,0,0]  (spconv_backbone.py:412)

    def head_names(self):
        return list(self.head_order) + ["hm"]

    def head_out(self, name):
        return self.num_class if name == "hm" else self.head_channels[name]


def init_state_dict(cfg: ModelConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Random-init weights under the REFERENCE's state_dict names and layouts (spconv-2.x conv
    weights (Cout,kD,kH,kW,Cin); torch Conv2d / ConvTranspose2d / BatchNorm). BN statistics are
    non-trivial so that folding errors would show up in parity tests."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    depth = 2  # sparse_shape z after conv_out for a 41-deep input; generic value computed by engine
    for L in layer_table.centerpoint_layers(cfg, depth=depth):
        fan = L.c_in * math.prod(L.ksize)
        sd[L.conv + ".weight"] = torch.randn(*L.weight_shape(), generator=g) * math.sqrt(2.0 / fan)
        if L.bias:
            sd[L.conv + ".bias"] = torch.randn(L.c_out, generator=g) * 0.05
        if L.bn:
            c = L.c_out
            sd[L.bn + ".weight"] = torch.rand(c, generator=g) * 0.5 + 0.75
            sd[L.bn + ".bias"] = torch.randn(c, generator=g) * 0.1
            sd[L.bn + ".running_mean"] = torch.randn(c, generator=g) * 0.1
            sd[L.bn + ".running_var"] = torch.rand(c, generator=g) * 0.5 + 0.75
            sd[L.bn + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
        if L.slot == ("head", "hm", 1):
            sd[L.conv + ".bias"] = torch.full((cfg.num_class,), -2.19)   # center_head.py:30
    return sd


def _fold_bn(sd, bn_name, eps, conv_bias=None):
    """Eval BatchNorm (+ preceding conv bias) as per-channel scale/shift."""
    w, b = sd[bn_name + ".weight"].double(), sd[bn_name + ".bias"].double()
    mean, var = sd[bn_name + ".running_mean"].double(), sd[bn_name + ".running_var"].double()
    scale = w / torch.sqrt(var + eps)
    shift = b - mean * scale
    if conv_bias is not None:
        shift = shift + conv_bias.double() * scale
    return scale.float(), shift.float()


class _Layer:
    __slots__ = ("w", "kv", "c_in", "c_out", "scale", "shift", "relu")

    def __init__(self, w_kio, scale, shift, relu, device):
        w_kio = w_kio.to(device=device, dtype=torch.float32).contiguous()
        self.kv, self.c_in, self.c_out = w_kio.shape
        self.w = ops.pack_weight(w_kio)
        self.scale = scale.to(device).contiguous() if scale is not None else None
        self.shift = shift.to(device).contiguous() if shift is not None else None
        self.relu = relu


class StridedStageChain:
    """The INDEX CHAIN of the four strided stages (output set -> row order -> rulebooks: 6-8 small launches and one count read-back per
    stage), which depends on site lists only, never on features. With a side stream it runs on a second HIP stream, ahead of the
    convolutions, and PIPELINED: a stage's output set is marked and counted (conv_outset_begin) as soon as the list it is marked from
    exists -- stage 2's at the start of the step, before the level-0 index, rulebook and the level-1 convs are queued; stage k + 1's as
    soon as stage k's list is emitted -- so that by the time the host asks for a count (conv_outset_end) the side stream has it, and the
    host is never away from the main stream for long. The index kernels overlap convolutions that do not fill the chip (one frame: 0.6
    of 3.0 ms of kernel time is index work). Without one: the same calls in the same order on the current stream. Same kernels, same
    results.

    The owner's `tables(stage, in_coords, in_index, in_shape, out_idx, out_index, out_shape)` builds what it needs of a stage (row
    order, rulebooks) and returns it; use: start() -> [level-0 index] -> index_ready() -> [level-1 convs] -> next() per stage, each
    after the previous stage's convs are queued (the count read-back inside can still block the host for a moment, and the main
    stream should have its work by then).

    Allocator safety across the streams: side-stream tensors read on the main stream (tables, lists, indexes) and main-stream
    tensors read on the side stream are held in `keep`, i.e. until the owner drops this chain for the NEXT step's -- and that one's
    start() makes the side stream wait for everything queued on the main stream so far: the caching allocator can hand a freed
    block to the other stream only after its readers ran."""

    def __init__(self, tables, batch, device, side_stream):
        self.tables, self.batch = tables, batch
        self.side = _lib.side_stream(device, "index") if side_stream else None     # (per current stream: an engine may be driven from several streams over its life)
        self.main = torch.cuda.current_stream(device) if side_stream else None
        self.keep = []
        self._stage = 0
        self._pending = self._after = None

    def _begin(self, coords, shape):
        return ops.conv_outset_begin(coords, self.batch, shape, *_DOWN[STRIDED_STAGES[self._stage]])

    def start(self, coords, shape):
        """level 0's site list exists: with a side stream, stage 2's output set is marked and counted beside what the main stream does next"""
        self._level = (coords, None, shape)
        if self.side is not None:
            self.side.wait_event(self.main.record_event())
            with torch.cuda.stream(self.side):
                self._pending = self._begin(coords, shape)

    def index_ready(self, index):
        """the level-0 site index (and its row order) is complete at this point of the main stream"""
        self._level = (self._level[0], index, self._level[2])
        self._after = self.main.record_event() if self.side is not None else None

    def next(self):
        """Queue the next stage's chain -- its conv_outset_end, the following stage's conv_outset_begin, the owner's tables -- and make
        the main stream wait for it. Returns what `tables` returned."""
        coords, index, shape = self._level
        if self._pending is None:                              # (no side stream: the first output set is marked here, after the level-1 convs)
            self._pending = self._begin(coords, shape)
        stage = STRIDED_STAGES[self._stage]
        with (torch.cuda.stream(self.side) if self.side is not None else contextlib.nullcontext()):
            out_idx, out_index, out_shape = ops.conv_outset_end(self._pending)
            if self._after is not None:
                self.side.wait_event(self._after)
                self._after = None
            self._stage += 1
            # (marked from the canonical list, whatever row order the owner gives the level)
            self._pending = self._begin(out_idx, out_shape) if self._stage < len(STRIDED_STAGES) else None
            T = self.tables(stage, coords, index, shape, out_idx, out_index, out_shape)
            if self.side is not None:
                self.main.wait_event(self.side.record_event())
        self.keep.append((self._level, self._pending, T))
        self._level = (out_idx, out_index, out_shape)
        return T


def bev_tables(cache, batch, h, w, device, transposed=False):
    """The pixel tables of BaseBEVBackbone's convs over (batch, h, w) maps, built once per shape; `transposed`: the stride-2 conv's
    transposed table as well (its input gradient)."""
    key = (batch, h, w)
    if key not in cache:
        t = {}
        t["s1"] = ops.rulebook_conv2d(batch, h, w, 3, 3, 1, 1, device)
        t["s2"] = ops.rulebook_conv2d(batch, h, w, 3, 3, 2, 1, device)
        h2, w2 = t["s2"][1], t["s2"][2]
        if transposed:
            t["s2_t"] = train_ops.rulebook_conv2d_transpose(batch, h, w, 3, 3, 2, 1, device)
        t["s1_half"] = ops.rulebook_conv2d(batch, h2, w2, 3, 3, 1, 1, device)
        # ConvTranspose2d(k=s=2) destination rows: tap (a,b) of coarse pixel (y,x) -> (2y+a, 2x+b)
        b_i = torch.arange(batch, device=device).view(-1, 1, 1)
        yy = torch.arange(h2, device=device).view(1, -1, 1)
        xx = torch.arange(w2, device=device).view(1, 1, -1)
        maps = [((b_i * h + 2 * yy + a) * w + 2 * xx + bb).reshape(-1) for a in range(2) for bb in range(2)]
        t["up2"] = torch.stack(maps).to(torch.int32).contiguous()
        cache[key] = t
    return cache[key]


class _StageTables(NamedTuple):
    """a strided stage's tables, as the engine's convs read them"""
    out_idx: torch.Tensor      # the level's site list in its row order
    out_index: object
    out_shape: list
    nbr_dn: torch.Tensor
    nbr: Optional[torch.Tensor]
    pairs_out: bool
    canon: Optional[tuple]     # (held: the chunk-wise tables were built from it)


class _PeakHead(NamedTuple):
    """a CenterHead cut at the peaks, as decode_and_nms takes it: the winners of every frame in their final order (ops.center_peaks)
    and the regression branches' hidden rows at the 9 sites around each (row order of ops.peak_rulebook)"""
    score: torch.Tensor
    cand: torch.Tensor
    ind: torch.Tensor
    hidden: torch.Tensor


class CenterPointEngine:
    """points [N, C] (device f32)  ->  {'pred_boxes','pred_scores','pred_labels'} per frame."""

    # BatchNorm eps: spconv_backbone.py:410, base_bev_backbone.py:38, nn.BatchNorm2d's default (center_head.py:24,78)
    BN_EPS = {"sparse": 1e-3, "bev": 1e-3, "head": 1e-5}

    def __init__(self, cfg: ModelConfig, state_dict: Dict[str, torch.Tensor], device="cuda", host_results=False):
        self.cfg = cfg
        self.device = torch.device(device)
        # host_results: the final boxes / scores / labels are returned as HOST tensors (the D2H of the padded result block
        # follows the step's one count read-back)
        self.host_results = bool(host_results)
        self.sd = state_dict
        self.voxelizer = ops.Voxelizer(cfg.voxel_size, cfg.point_cloud_range, cfg.num_point_features,
                                       cfg.max_points_per_voxel, cfg.max_voxels, device=self.device)
        self._voxelizers = [self.voxelizer]
        self._group_voxelizers = []
        self._bev_cache = {}
        self.last_head_at_peaks = False    # did the last step evaluate the regression branches at the peaks only (diagnostics, tests)
        self._peaks = None                 # (a CenterHead's layers cut at the peaks, _build_head; other dense heads leave it None)
        self.head_at_peaks = bool(cfg.head_at_peaks) and os.environ.get("CPD_HEAD_AT_PEAKS", "1") != "0"
        self.guard = RangeGuard(self.RANGE_STICKY_STEPS)
        self._pool = None                  # the step's absmax blocks; None: nothing is recorded (another arithmetic, or the guard switched off)
        if cfg.conv_math == "f16x2" and cfg.range_guard:
            self._pool = BlockPool("range guard: this model launches more convolutions per step than the %d absmax blocks the engine "
                                   "sized from its config (engine._range_reset)")
        self._range_new = self._pool.new_block if self._pool is not None else (lambda: None)     # the block of one conv launch
        self._rb = None                    # block of the tensor the NEXT conv reads (_conv)
        self._rb_stage = None              # "backbone" between backbone3d and the bev_and_head that goes on from its blocks
        self._dense_map = None             # the persistent BEV map of the step in flight, until its one reader is queued
        self._export_pair_levels = False   # forward(pair_levels=True): exported levels stay fp16-pair rows
        self.encoded_pairs = False         # did the last backbone3d leave its stride-8 output in pair rows
        self._index_chain = None           # the step's StridedStageChain (held until the next step replaces it)
        self.last_result_block = None      # (boxes [B, K, 7], scores, labels i64, counts i32 [B]) of the last step, on the device
        self._build_layers()

    # ------------------------------------------------------------------ weights
    def _folded(self, L):
        """a layer_table record -> (w_kio, scale, shift): the reference's weights in our layout, eval BatchNorm (+ conv bias) folded"""
        sd = self.sd
        w = L.kio(sd[L.conv + ".weight"], self.cfg.out_features, self._final_shape()[0])
        bias = sd.get(L.conv + ".bias") if L.bias else None
        if L.bn is None:
            return w, None, bias
        s, t = _fold_bn(sd, L.bn, self.BN_EPS[L.group], bias)
        return w, s.repeat(L.up * L.up), t.repeat(L.up * L.up)      # (a deblock's u*u taps are column groups of one GEMM)

    def _build_layers(self):
        at = {L.slot: _Layer(*self._folded(L), L.relu, self.device) for L in layer_table.centerpoint_layers(self.cfg) if L.group != "head"}
        self.sparse, self.bev_levels = layer_table.sparse_and_bev(self.cfg, at)
        self._build_head()

    def _build_head(self):
        """CenterHead's convolutions (center_head.py:73-94); a subclass with another dense head (cpd_amd/anchor_engine.py) overrides this,
        `_head_rows` and `decode_and_nms`."""
        first, last = [], []
        for L in layer_table.centerpoint_layers(self.cfg):
            if L.slot == ("shared",):
                self.shared = _Layer(*self._folded(L), L.relu, self.device)
            elif L.slot[0] == "head":
                (last if L.slot[2] else first).append(self._folded(L))
        # the five SeparateHead branches: first convs fused along Cout, second convs block-diagonal
        (lw, _, lb) = zip(*last)
        w1, s1, t1, w2, b2, slices = layer_table.fuse_branches(*zip(*first), lw, lb)
        self.head_slices = dict(zip(self.cfg.head_names(), slices))
        self.head1 = _Layer(w1, s1, t1, True, self.device)
        self.head2 = _Layer(w2, None, b2, False, self.device)
        self.head_ld = 16 * ((w2.shape[2] + 15) // 16)
        # ... and cut at the peaks (ModelConfig.head_at_peaks): the hm branch on its own, the regression branches' first convs side by
        # side, their last convs as the fp32 image of the native finish
        names = self.cfg.head_names()
        P = layer_table.split_branches_at(*zip(*first), lw, lb, names.index("hm"))
        hm_ld = 16 * ((self.cfg.num_class + 15) // 16)
        w_last, b_last = P["rest2"]
        off = dict(zip([n for n in names if n != "hm"], (c0 for c0, _ in P["rest_slices"])))
        self._peaks = dict(head1_hm=_Layer(*P["keep1"], True, self.device), head2_hm=_Layer(P["keep2"][0], None, P["keep2"][1], False, self.device),
                           reg1=_Layer(*P["rest1"], True, self.device), hm_ld=hm_ld,
                           w_last=w_last.to(device=self.device, dtype=torch.float32).contiguous(),
                           b_last=b_last.to(device=self.device, dtype=torch.float32).contiguous(),
                           offsets=[off["center"], off["center_z"], off["dim"], off["rot"]])

    def _final_shape(self):
        return final_shape(self.cfg)

    def _side_stream(self):
        return _lib.side_stream(self.device, "index")      # (per current stream: an engine may be driven from several streams over its life)

    # ------------------------------------------------------------------ forward pieces
    # Range guard of the f16x2 path (range_guard.py). Every conv epilogue raises an absmax block of the step's pool to max |out| (a wave
    # reduction + a rarely issued atomic: free). OPTIMISTIC pass: the layers run their unscaled kernels and only RECORD. GUARDED pass
    # (guard.scaled): each layer also takes its input's block as `in_absmax` (the `*_f16s_*` kernels pre-scale by a power of two).
    # `self._rb` = block of the tensor the NEXT conv reads; a _conv call consumes it and replaces it by the block its epilogue fills.
    def _range_reset(self):
        self._rb = None
        if self._pool is not None:
            # one block per conv launch of a step: 20 sparse layers + conv_out, the BEV levels' convs, the concat buffer,
            # shared conv + the two head launches (three with the head cut at the peaks; + slack for callers that run the stages on their own)
            self._pool.reset(21 + sum(k + 1 for k in self.cfg.bev_layer_nums) + 1 + 3 + 16, self.device)

    RANGE_STICKY_STEPS = 16       # guarded steps that follow a re-run before the engine tries the unguarded kernels again
    range_reruns = property(lambda self: self.guard.reruns, lambda self, n: setattr(self.guard, "reruns", n))
    range_guarded_steps = property(lambda self: self.guard.guarded_steps)
    _guard_left = property(lambda self: self.guard.left)

    def _range_exceeded_flag(self):
        """device int32 [1] riding with the step's count read-back; None when nothing is recorded. Optimistic step: 1 when some
        recorded activation is >= 2^15 (or NaN / inf) -> the step is re-run guarded. Guarded step: 1 while some activation is
        still >= 2^14 -> the engine stays guarded (hysteresis: it returns to the unguarded kernels only after
        RANGE_STICKY_STEPS consecutive steps well inside fp16's range)."""
        if self._pool is None:
            return None
        return self._pool.flag(GUARDED_BITS if self.guard.scaled else OPTIMISTIC_BITS)

    def _conv(self, layer, x, nbr, n_out, residual=None, out=None, out_row_map=None, out_col_group=0, dense=False, out_rb="new",
              in_pairs=False, out_pairs=False, res_pairs=False):
        rb_in = self._rb if self.guard.scaled else None
        rb_out = self._range_new() if out_rb == "new" else out_rb
        y = ops.gather_conv(x, layer.c_in, layer.w, nbr, layer.kv, n_out, layer.c_out, layer.scale, layer.shift,
                            residual, layer.relu, out=out, out_row_map=out_row_map, out_col_group=out_col_group,
                            dense=dense, math=self.cfg.conv_math, in_absmax=rb_in, out_absmax=rb_out,
                            in_pairs=in_pairs, out_pairs=out_pairs, res_pairs=res_pairs)
        self._rb = rb_out
        return y

    def _blocks(self, blocks, x, nbr, pairs=False):
        n = x.shape[0]
        for c1, c2 in blocks:                      # SparseBasicBlock, spconv_backbone.py:120-136
            y = self._conv(c1, x, nbr, n, in_pairs=pairs, out_pairs=pairs)
            x = self._conv(c2, y, nbr, n, residual=x, in_pairs=pairs, out_pairs=pairs, res_pairs=pairs)
        return x

    def backbone3d(self, feats, coords, batch, index=None, pair_rows=False, export_levels=True, canonical0=False, dense_pairs=False):
        """VoxelResBackBone8x.forward (spconv_backbone.py:502-558). Returns per-level
        {name: (features, indices, spatial_shape)} and the stride-8 output. `index`: the level-0 site index when the
        voxelizer already built it (cpd_voxelize_batch_index). `pair_rows`: levels 2-4 keep their activations as fp16-pair rows
        between layers (ModelConfig.pair_rows; f16x2 only); the returned level features are fp32 either way when
        `export_levels` (decoded copies), else whatever the layers left."""
        pairs = bool(pair_rows) and self.cfg.conv_math == "f16x2"
        want = (lambda name: name in export_levels) if isinstance(export_levels, (tuple, list, set)) else (lambda name: bool(export_levels))
        self.level_indexes = {}                               # name -> SiteIndex of the level (in the level's row order)
        L = self.sparse
        shape = self.cfg.sparse_shape
        side = self.cfg.index_side_stream and feats.is_cuda and batch <= self.cfg.index_side_stream_max_frames

        def tables(stage, in_coords, index, in_shape, out_idx, out_index, out_shape):
            """everything of a strided stage that depends on the site lists only: its row order and both rulebooks"""
            k, s, pd = _DOWN[stage]
            if stage == "conv_out":
                return _StageTables(out_idx, out_index, out_shape, ops.rulebook_conv(out_idx, index, k, s, pd), None, False, None)
            out_c = out_idx
            # "bricks" per level: only where the staged kernel is used (plan_channels: the widths it wins at); other levels keep "taps"
            c_lvl = L[stage + ".down"].c_out
            use_plan = self.cfg.plan_rulebooks and pairs and c_lvl in self.cfg.plan_channels
            bricks = self.cfg.row_order == "bricks" and out_idx.shape[0] >= self.cfg.row_order_min_rows and (use_plan or not self.cfg.plan_rulebooks)
            canon = None                      # (canonical list, order, chunk) of a chunk-ordered level: its tables are built chunk-wise
            if bricks:
                out_idx, _, old_to_new = ops.order_rows_bricks(out_c, out_index, brick=self.cfg.row_order_brick, tile_rows=self.cfg.plan_tile_rows)
                out_index.set_order(old_to_new)
            elif self.cfg.row_order in ("taps", "bricks") and out_idx.shape[0] >= self.cfg.row_order_min_rows:
                # rows of the level sorted, chunk by chunk, by their neighbour pattern (ops.order_rows_by_taps): the level's
                # site list in the new order + the rank -> row map installed in its index re-order everything that follows
                # (both rulebooks, the features, the exported level) without any kernel knowing
                out_idx, _, old_to_new = ops.order_rows_by_taps(out_c, out_index, chunk_rows=self.cfg.row_order_chunk)
                out_index.set_order(old_to_new)
                if self.cfg.chunked_rulebooks:
                    canon = (out_c, old_to_new, self.cfg.row_order_chunk)
            nbr_dn = ops.rulebook_conv(out_idx, index, k, s, pd, canonical=canon)
            # (pair rows are read through the row-wave kernel's 4 GB buffer resource: a level that large stays fp32)
            pairs_out = pairs and out_idx.shape[0] * c_lvl * 4 < 0xfffff000
            nbr = ops.rulebook_subm(out_idx, out_index, canonical=canon)
            if bricks and pairs_out and use_plan:
                ops.rulebook_plan(nbr, self.cfg.plan_tile_rows)  # the level's four SubM convs: the staged row-wave kernel
            return _StageTables(out_idx, out_index, out_shape, nbr_dn, nbr, pairs_out, canon)

        chain = self._index_chain = StridedStageChain(tables, batch, self.device, side)     # (the previous step's is dropped here)
        chain.start(coords, shape)
        if index is None:
            index = ops.SiteIndex.build(coords, batch, shape)
        coords_c0, canon0 = coords, None
        if canonical0 and self.cfg.row_order == "taps" and self.cfg.row_order_level0 and coords.shape[0] >= self.cfg.row_order_min_rows:
            # level 0 in tap-pattern order too (round 4): its rows have 4.3 of 27 neighbours on average, and a canonical 16-row group
            # executes 2.2x the (group, tap) pairs its rows need -- 1.3x after the sort (tools/unique_probe.py). `canonical0`: the
            # voxelizer delivered canonical rows and a canonical index (rank = row), which is what the sort and the map need.
            coords, n2o, o2n = ops.order_rows_by_taps(coords_c0, index, chunk_rows=self.cfg.row_order_chunk)
            index.set_order(o2n)
            feats = feats.index_select(0, n2o.long())
            if self.cfg.chunked_rulebooks:
                canon0 = (coords_c0, o2n, self.cfg.row_order_chunk)
        pairs16 = pairs and self.cfg.pair_rows_level1
        chain.index_ready(index)
        nbr = ops.rulebook_subm(coords, index, canonical=canon0)               # 'subm1' and 'res1' are the same L0 table
        self._range_reset()                                  # (the 5-channel input layer runs on the fp32 pipe: no block for `feats`)
        # level 1 (16 channels): with pair rows its layers run the K = 16 split-fp16 MFMA on 16-channel pair rows (three products of
        # 16 matrix cycles instead of four fp32 MFMAs of 32); the 5-channel input layer stays on the fp32 pipe and writes the first pairs
        x = self._conv(L["conv_input"], feats, nbr, coords.shape[0], out_pairs=pairs16)
        x = self._blocks(L["conv1"], x, nbr, pairs=pairs16)
        raw = self._export_pair_levels                        # exported levels stay fp16-pair rows, wrapped in ops.PairRows (the RoI pooling's first GEMM reads them as they are)

        def export(t, is_pairs, name):
            if not (is_pairs and want(name)):
                return t
            if raw and t.shape[1] % 32 == 0:
                return ops.PairRows(t)
            return ops.pairs_to_rows(t)
        levels = {"x_conv1": (export(x, pairs16, "x_conv1"), coords, shape)}
        self.level_indexes["x_conv1"] = index
        pairs_in = pairs16                 # (what conv2.down reads)
        T = chain.next()
        for i, stage in enumerate(STRIDED_STAGES, start=2):
            out_idx, out_shape = T.out_idx, T.out_shape
            if stage == "conv_out":
                break
            pairs_out = T.pairs_out
            x = self._conv(L[stage + ".down"], x, T.nbr_dn, out_idx.shape[0], in_pairs=pairs_in, out_pairs=pairs_out)
            x = self._blocks(L[stage], x, T.nbr, pairs=pairs_out)
            pairs_in = pairs_out
            levels["x_conv%d" % i] = (export(x, pairs_in, "x_conv%d" % i), out_idx, out_shape)
            self.level_indexes["x_conv%d" % i] = T.out_index
            T = chain.next()
        # (dense_pairs: the stride-8 output stays in pair rows -- densify is a copy of row bytes, so the BEV map it builds is a pair-row map)
        x = self._conv(L["conv_out"], x, T.nbr_dn, out_idx.shape[0], in_pairs=pairs_in, out_pairs=bool(dense_pairs) and pairs_in)
        self.encoded_pairs = bool(dense_pairs) and pairs_in
        self._rb_stage = "backbone"                            # the densified map inherits this output's range block
        return levels, (x, out_idx, out_shape)

    def dense_pairs_ok(self, batch, h, w):
        """can this batch run its dense half on fp16-pair maps? Every 3 x 3 / stride 1 layer must take one of the window tiles the pair
        kernels exist for (128 x 128, 256 x 64, 256 x 16: cpd_conv3x3_rows_tile), the strided / deblock GEMMs need 128-column tiles,
        and every map must stay below the 4 GB a buffer resource addresses."""
        cfg = self.cfg
        if not (cfg.pair_rows_dense and cfg.pair_rows and cfg.conv_math == "f16x2"):
            return False
        key = ("dense_pairs", batch, h, w)
        if key in self._bev_cache:
            return self._bev_cache[key]
        ok = True
        cur_h, cur_w = h, w
        widest = self.bev_levels[0][0][0].c_in
        for lvl, (convs, de, u, c_up) in enumerate(self.bev_levels):
            stride = cfg.bev_layer_strides[lvl]
            if stride == 2:
                cur_h, cur_w = (cur_h + 2 - 3) // 2 + 1, (cur_w + 2 - 3) // 2 + 1
                ok = ok and convs[0].c_out % 128 == 0 and convs[0].c_in % 32 == 0
            for cv in (convs if stride == 1 else convs[1:]):
                ok = ok and ops.conv3x3_rows_tile(batch, cur_h, cur_w, cv.c_in, cv.c_out) in ((128, 128), (128, 64))
            ok = ok and de.c_out % 128 == 0 and c_up % 32 == 0
            widest = max(widest, max(cv.c_out for cv in convs))
        c_cat = sum(cfg.bev_num_upsample_filters)
        ok = ok and self._head_pairs_ok(batch, h, w, c_cat)
        widest = max(widest, c_cat, getattr(getattr(self, "head1", None), "c_out", 0))
        ok = ok and batch * h * w * widest * 4 + (w + 300) * widest * 4 < 0xfff00000
        self._bev_cache[key] = bool(ok)
        return bool(ok)

    def _head_pairs_ok(self, batch, h, w, c_cat):
        return (ops.conv3x3_rows_tile(batch, h, w, c_cat, self.shared.c_out) in ((256, 64), (128, 64)) and
                ops.conv3x3_rows_tile(batch, h, w, self.head1.c_in, self.head1.c_out) in ((256, 64), (128, 64)) and
                ops.conv3x3_rows_tile(batch, h, w, self.head2.c_in, self.head2.c_out) in ((256, 16), (128, 16)))

    def _head_at_peaks_ok(self, batch, h, w):
        """does this batch shape take the head cut at the peaks (ModelConfig.head_at_peaks)? Only where the hm branch's two layers get
        the window kernel and the very tile they have inside the fused layers (64 -> 64 on head1's 64-column tile, 64 -> num_class on
        head2's 16-column tile, the hm columns a whole tile of head1): the same kernel on the same tile does the same arithmetic, so
        the scores are those of the full maps bit for bit. Any other shape keeps the full maps."""
        P, cfg = self._peaks, self.cfg
        if P is None or not self.head_at_peaks or batch < cfg.head_at_peaks_min_frames:
            return False
        key = ("head_at_peaks", batch, h, w)
        if key not in self._bev_cache:
            k = cfg.max_obj_per_sample
            tile = lambda L: ops.conv3x3_rows_tile(batch, h, w, L.c_in, L.c_out, cfg.conv_math) if cfg.conv_math in ("f16x2", "bf16x3") else None
            t1, t2 = tile(self.head1), tile(self.head2)
            hm_col = cfg.head_names().index("hm") * P["head1_hm"].c_out          # first hidden column of the hm branch in head1
            self._bev_cache[key] = bool(
                t1 is not None and t2 is not None and t1 == tile(P["head1_hm"]) and t2 == tile(P["head2_hm"]) and
                P["head1_hm"].c_out == t1[1] and hm_col % t1[1] == 0 and k <= 1024 and k <= h * w and
                batch * k * 9 * 4 * P["reg1"].c_out < 0xfff00000)
        return self._bev_cache[key]

    def bev_and_head(self, dense_rows, batch, h, w, pairs=False, at_peaks=False):
        """BaseBEVBackbone.forward (base_bev_backbone.py:85-122) + CenterHead convs
        (center_head.py:323-330) on channels-last rows [batch*h*w, C]. `pairs`: `dense_rows` and every map up to the head's hidden
        layer are fp16-pair maps (ModelConfig.pair_rows_dense); the returned concat map is then a pair map, the head rows are fp32.
        `at_peaks` (forward() only, where _head_at_peaks_ok): instead of the head rows, what decode_and_nms takes of a head cut at the
        peaks (_PeakHead)."""
        cfg = self.cfg
        pk = dict(in_pairs=True, out_pairs=True) if pairs else {}
        T = bev_tables(self._bev_cache, batch, h, w, self.device)
        if self._rb_stage != "backbone":                       # called on its own (tests, tools): the input's range is unknown
            self._range_reset()
        self._rb_stage = None
        cat_rb = self._range_new()                             # ONE block for the concat buffer: both deblocks raise it
        n_full = batch * h * w
        c_cat = sum(cfg.bev_num_upsample_filters)
        cat = torch.empty((n_full, c_cat), dtype=torch.float32, device=self.device)
        x = dense_rows
        col = 0
        cur_h, cur_w = h, w
        side = self._side_stream() if (cfg.index_side_stream and cfg.deblock_side_stream and dense_rows.is_cuda
                                       and batch <= cfg.deblock_side_stream_max_frames) else None
        main = torch.cuda.current_stream(self.device) if side is not None else None
        held, joins = [], []
        for lvl, (convs, de, u, c_up) in enumerate(self.bev_levels):
            stride = cfg.bev_layer_strides[lvl]
            if stride == 1:
                nbr0, ho, wo = T["s1"] if (cur_h, cur_w) == (h, w) else T["s1_half"]
            elif stride == 2 and (cur_h, cur_w) == (h, w):
                nbr0, ho, wo = T["s2"]
            else:
                raise NotImplementedError("BEV stride pattern outside the shipped configs")
            n_lvl = batch * ho * wo
            x = self._conv(convs[0], x, nbr0, n_lvl, dense=True, **pk)
            if lvl == 0 and self._dense_map is not None:
                self._dense_map.clear()                        # the densified map's only reader is queued: its rows go back to zero
                self._dense_map = None
            nbr_same = T["s1"][0] if (ho, wo) == (h, w) else T["s1_half"][0]
            for cv in convs[1:]:
                x = self._conv(cv, x, nbr_same, n_lvl, dense=True, **pk)
            cur_h, cur_w = ho, wo
            dst = cat[:, col:col + c_up]
            x_rb = self._rb                                    # the next level goes on from x, not from the deblock's output
            # a deblock that is not the last one has a whole level of convolutions between it and its reader (the shared conv): with the
            # side stream it runs beside them -- an HBM-bound GEMM (2.6 GB per 48 frames) under matrix-bound window convs
            aside = side is not None and lvl + 1 < len(self.bev_levels)
            if aside:
                ev = main.record_event()
                held.append(x)                                 # (main-stream tensor read on the side stream: alive until the join below)
            with (torch.cuda.stream(side) if aside else contextlib.nullcontext()):
                if aside:
                    side.wait_event(ev)
                if u == 1:
                    self._conv(de, x, None, n_lvl, out=dst, dense=True, out_rb=cat_rb, **pk)
                elif u == 2 and (ho * 2, wo * 2) == (h, w):
                    self._conv(de, x, None, n_lvl, out=dst, out_row_map=T["up2"], out_col_group=c_up, dense=True, out_rb=cat_rb, **pk)
                else:
                    raise NotImplementedError("upsample stride outside the shipped configs")
                if aside:
                    joins.append(side.record_event())
            self._rb = x_rb
            col += c_up
        for ev in joins:
            main.wait_event(ev)
        self._rb = cat_rb
        if at_peaks:
            return cat, self._head_rows_at_peaks(cat, batch, h, w, T, pairs)
        return cat, self._head_rows(cat, batch, h, w, T, pairs)

    def _head_rows(self, cat, batch, h, w, T, pairs):
        """the dense head's convolutions on the concat map's rows -> what decode_and_nms takes (CenterHead: the head rows)"""
        pk = dict(in_pairs=True, out_pairs=True) if pairs else {}
        n_full = batch * h * w
        s = self._conv(self.shared, cat, T["s1"][0], n_full, dense=True, **pk)
        h1 = self._conv(self.head1, s, T["s1"][0], n_full, dense=True, **pk)
        out = torch.empty((n_full, self.head_ld), dtype=torch.float32, device=self.device)
        self._conv(self.head2, h1, T["s1"][0], n_full, out=out, dense=pairs, in_pairs=pairs)
        return out

    def _head_rows_at_peaks(self, cat, batch, h, w, T, pairs):
        """the head cut at the peaks: shared conv and the hm branch over every pixel (the window kernels, as in _head_rows), the
        selection, then the regression branches' first convs over the 9 hidden sites around each winner -- one gather_conv launch over
        the shared map's rows. Nothing is read back; every shape is fixed by (batch, max_obj_per_sample, h, w)."""
        P, cfg = self._peaks, self.cfg
        pk = dict(in_pairs=True, out_pairs=True) if pairs else {}
        n_full = batch * h * w
        k = cfg.max_obj_per_sample
        s = self._conv(self.shared, cat, T["s1"][0], n_full, dense=True, **pk)
        s_rb = self._rb                                        # the shared map has two readers
        h1 = self._conv(P["head1_hm"], s, T["s1"][0], n_full, dense=True, **pk)
        hm = torch.empty((n_full, P["hm_ld"]), dtype=torch.float32, device=self.device)
        self._conv(P["head2_hm"], h1, T["s1"][0], n_full, out=hm, dense=pairs, in_pairs=pairs)
        score, cand, ind = ops.center_peaks(hm, P["hm_ld"], 1, cfg.num_class, h, w, k, batch=batch, sample_stride=h * w * P["hm_ld"])
        nbr = ops.peak_rulebook(ind, h, w)
        self._rb = s_rb
        hidden = self._conv(P["reg1"], s, nbr, batch * k * 9, in_pairs=pairs)
        return _PeakHead(score, cand, ind, hidden)

    def decode_and_nms(self, head_rows, batch, h, w, raw=False):
        """generate_predicted_boxes (center_head.py:252-303) + class_agnostic_nms
        (model_nms_utils.py:115-134) for all samples of the batch: five launches, nothing read back
        until the final per-sample counts. `head_rows`: the head rows, or the _PeakHead of a head cut at the peaks."""
        cfg = self.cfg
        ld = self.head_ld
        sl = self.head_slices
        base = head_rows
        if isinstance(head_rows, _PeakHead):
            P = self._peaks
            boxes, scores, labels, counts = ops.center_decode_at_peaks(
                head_rows.score, head_rows.cand, head_rows.ind, head_rows.hidden, P["reg1"].c_out, P["w_last"], P["b_last"], P["offsets"],
                cfg.num_class, h, w, float(cfg.feature_map_stride), cfg.voxel_size[:2], cfg.point_cloud_range[:2],
                cfg.post_center_limit_range, cfg.score_thresh)
        else:
            boxes, scores, labels, counts = ops.center_decode(
                base[:, sl["hm"][0]:], base[:, sl["center"][0]:], base[:, sl["center_z"][0]:], base[:, sl["dim"][0]:],
                base[:, sl["rot"][0]:], ld, 1, cfg.num_class, h, w, cfg.max_obj_per_sample, float(cfg.feature_map_stride),
                cfg.voxel_size[:2], cfg.point_cloud_range[:2], cfg.post_center_limit_range, cfg.score_thresh, sync=False,
                batch=batch, sample_stride=h * w * ld)
        # scores come out sorted descending (top-K order survives the masks), so the
        # topk(NMS_PRE_MAXSIZE) + sort inside nms_gpu are identities (K = 500 <= 4096)
        assert cfg.max_obj_per_sample <= cfg.nms_pre_maxsize
        keep, num_keep = ops.nms_batch(boxes, counts, cfg.nms_thresh)
        flag = self._range_exceeded_flag()        # the range guard's verdict travels with the counts: no extra synchronisation
        # counts, the verdict and the padded boxes / scores / labels are ONE device block: with host results one blocking copy brings a
        # step's whole output over (they were four: the counts, then three tensors at ~25 us of synchronisation each)
        ob, os_, ol, on, blk = ops.select_boxes(boxes, scores, labels, keep, num_keep, cfg.nms_post_maxsize, label_offset=1,
                                                packed=True, extra_ints=1)
        lay = blk._cpd_layout
        hdr = blk[:4 * lay["n_hdr"]].view(torch.int32)
        if flag is not None:
            hdr[batch:batch + 1].copy_(flag)
        whole = self.host_results and not raw
        # (blocking copies. Asynchronous copies into pinned memory queued on the compute stream were measured 5-8 ms per step SLOWER on
        # MI355X / ROCm 7.2 -- tools/d2h_probe.py -- whatever the wait that followed them: event, stream or a later blocking read.)
        host = blk.cpu() if whole else None       # the one host read-back of the stage
        ns = (ops.unpack_boxes(host, lay)[0] if whole else hdr).tolist()
        if self.guard.verdict(flag is not None and ns[batch]):
            return None                           # forward() runs the step again, guarded
        ns = ns[:batch]
        self.last_result_block = (ob, os_, ol, on)     # the step's padded device block and its device counts (cpd_amd/tta.py goes on from it)
        if raw:                                   # the padded device block + per-frame counts (the two-stage engine's proposals)
            return ob, os_, ol, ns
        if whole:
            _, ob, os_, ol = ops.unpack_boxes(host, lay)
        return [{"pred_boxes": ob[b, :ns[b]], "pred_scores": os_[b, :ns[b]], "pred_labels": ol[b, :ns[b]]}
                for b in range(batch)]

    # ------------------------------------------------------------------ whole frame(s)
    @torch.no_grad()
    def forward(self, points_list, return_intermediates=False, proposals=None, pair_levels=False):
        """points_list: list of [N_i, C] device tensors (one per frame of the batch).
        pair_levels (with proposals): the exported levels of >= 32 channels are left as fp16-pair rows (ops.PairRows instead of a tensor)
        when the step ran on pair rows -- what roi_pool's first GEMM takes directly; default fp32 rows.
        proposals = a collection of level names: the first stage of a two-stage detector -- returns
        (boxes [B, cap, 7], scores, labels i64 (1-based), per-frame counts (host list), levels) with the named levels' features
        exported as fp32 rows and their site indexes in self.level_indexes; nothing but the counts leaves the device."""
        if isinstance(points_list, torch.Tensor):
            points_list = [points_list]
        batch = len(points_list)
        index0 = None
        canonical0 = False
        z_extra = self.cfg.sparse_shape[0] - self.cfg.grid_zyx[0]
        if batch >= self.cfg.batched_voxelizer_min_frames and self.voxelizer.batch_supported(batch, z_extra):
            # one set of voxelizer launches for the whole batch; rows come out frame after frame; the voxelizer's occupancy
            # bitmap / prefix / rank -> row map ARE the level-0 site index of the backbone
            n_pts = sum(int(p.shape[0]) for p in points_list)
            canonical = self.cfg.voxel_row_order == "canonical" and batch * self.cfg.max_voxels >= n_pts
            _, coords, _, feats, nvox, index0 = self.voxelizer.batch(points_list, index_z_extra=z_extra, canonical=canonical)
            counts = nvox.tolist()                          # the one read-back: per-frame counts + total
            if canonical and max(counts[:batch]) > self.cfg.max_voxels:
                # a frame above its max_voxels cap: which voxels survive is defined on first-appearance order -- the exact path
                _, coords, _, feats, nvox, index0 = self.voxelizer.batch(points_list, index_z_extra=z_extra)
                counts = nvox.tolist()
            total = counts[batch]
            feats, coords = feats[:total], coords[:total]
            canonical0 = canonical and max(counts[:batch]) <= self.cfg.max_voxels
        elif batch > 1 and self.voxelizer.batch_supported(self.cfg.voxelizer_group, z_extra):
            # more frames than one batched-voxelizer call takes: groups of `voxelizer_group` frames, one voxelizer
            # (workspace) per group, rows concatenated with the frame index offset; the level-0 index is built over the whole list
            g = self.cfg.voxelizer_group
            groups = [points_list[i:i + g] for i in range(0, batch, g)]
            if len(groups[-1]) == 1:                        # e.g. batch = g + 1: the batched call wants >= 2 frames -- borrow one
                groups[-1].insert(0, groups[-2].pop())
            while len(self._group_voxelizers) < len(groups):
                self._group_voxelizers.append(ops.Voxelizer(self.cfg.voxel_size, self.cfg.point_cloud_range, self.cfg.num_point_features,
                                                            self.cfg.max_points_per_voxel, self.cfg.max_voxels, device=self.device))
            outs = [vz.batch(grp) for vz, grp in zip(self._group_voxelizers, groups)]
            totals = torch.stack([o[4][len(grp)] for o, grp in zip(outs, groups)]).tolist()       # the one read-back
            feats = torch.cat([o[3][:m] for o, m in zip(outs, totals)])
            parts, first = [], 0
            for o, m, grp in zip(outs, totals, groups):
                c = o[1][:m].clone()
                c[:, 0] += first                            # frame index within the whole batch
                parts.append(c)
                first += len(grp)
            coords = torch.cat(parts)
        else:
            while len(self._voxelizers) < batch:           # one workspace per in-flight frame of the batch
                self._voxelizers.append(ops.Voxelizer(self.cfg.voxel_size, self.cfg.point_cloud_range,
                                                      self.cfg.num_point_features, self.cfg.max_points_per_voxel,
                                                      self.cfg.max_voxels, device=self.device))
            outs = [self._voxelizers[b](pts, batch_idx=b, coord_cols=4, want_voxels=False, want_mean=True, sync=False)
                    for b, pts in enumerate(points_list)]
            ms = torch.cat([o[4] for o in outs]).tolist() if batch > 1 else [int(outs[0][4].item())]   # one read-back
            feats = torch.cat([o[3][:m] for o, m in zip(outs, ms)]) if batch > 1 else outs[0][3][:ms[0]]
            coords = torch.cat([o[1][:m] for o, m in zip(outs, ms)]) if batch > 1 else outs[0][1][:ms[0]]
        guard = self.guard
        guard.begin_step()                                   # guarded from the start while the stay after a re-run lasts (range_guard.py)
        fd, fh, fw = self._final_shape()
        self._export_pair_levels = bool(pair_levels) and proposals is not None
        while True:
            dp = (not guard.scaled) and self.dense_pairs_ok(batch, fh, fw)
            levels, (x, out_idx, out_shape) = self.backbone3d(feats, coords, batch, index=index0, canonical0=canonical0,
                                                              export_levels=proposals if proposals is not None else return_intermediates,
                                                              pair_rows=self.cfg.pair_rows and not guard.scaled, dense_pairs=dp)
            d, h, w = out_shape
            dp = dp and self.encoded_pairs
            # the BEV map: a persistent pre-zeroed buffer per batch shape -- the occupied rows (12 % at this level) are scattered in and,
            # once its one reader (the first BEV conv) is queued, zeroed again: no 36 MB-per-frame clear (round 5). Callers that keep the
            # map (return_intermediates) get a fresh tensor
            dmap = None
            if self.cfg.persistent_dense_map and not return_intermediates:
                key = ("dense_map", d, h, w, x.shape[1])
                dmap = self._bev_cache.get(key)
                if dmap is None or dmap.batch < batch:      # one map, sized for the largest batch seen; smaller batches use its leading frames
                    dmap = self._bev_cache[key] = ops.DenseMap(batch, out_shape, x.shape[1], self.device)
                dense = dmap.scatter(x, out_idx, batch).view(batch * h * w, d * x.shape[1])
            else:
                dense = ops.densify_nhwc(x, out_idx, batch, out_shape).view(batch * h * w, d * x.shape[1])
            self._dense_map = dmap
            # (callers that get the head rows back keep the full maps)
            peaks = self.last_head_at_peaks = (not return_intermediates) and self._head_at_peaks_ok(batch, h, w)
            cat, head = self.bev_and_head(dense, batch, h, w, pairs=dp, at_peaks=peaks)
            results = self.decode_and_nms(head, batch, h, w, raw=proposals is not None)
            if results is not None:
                break
            guard.trip()     # an activation left fp16's safe range: the same step with every layer pre-scaling its input (exact), range_guard.py
        guard.end_step()
        if proposals is not None:
            return results + (levels,)
        if return_intermediates:
            if dp:                                         # exported tensors are fp32 (h + l is exact)
                x, dense, cat = ops.pairs_to_rows(x), ops.pairs_to_rows(dense), ops.pairs_to_rows(cat)
            return results, dict(voxel_features=feats, voxel_coords=coords, levels=levels,
                                 encoded=(x, out_idx, out_shape), spatial_features_nhwc=dense, bev_cat=cat,
                                 head_rows=head, dense_pairs=dp)
        return results

    __call__ = forward
