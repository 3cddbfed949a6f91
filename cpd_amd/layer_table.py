"""The one map from the reference's parameter names and layouts to this package's: which convolutions CenterPoint has
(MeanVFE -> VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone -> CenterHead), what each is called in a reference
state_dict, and how its weights become a `[kv, Cin, Cout]` image and back. The inference engine, the trainer (both directions)
and init_state_dict walk `centerpoint_layers`; the fused heads of the module path share `fuse_branches`. Pure torch on the
host: permutes and reshapes only, nothing here launches a kernel.
"""
from typing import NamedTuple, Optional, Tuple

import torch

from . import ops

# Sparse stages of VoxelResBackBone8x (spconv_backbone.py:414-455): name -> (ksize, stride, pad)
_DOWN = {
    "conv2": ([3, 3, 3], [2, 2, 2], [1, 1, 1]),
    "conv3": ([3, 3, 3], [2, 2, 2], [1, 1, 1]),
    "conv4": ([3, 3, 3], [2, 2, 2], [0, 1, 1]),
    "conv_out": ([3, 1, 1], [2, 1, 1], [0, 0, 0]),
}
STRIDED_STAGES = ("conv2", "conv3", "conv4", "conv_out")


def final_shape(cfg):
    """(depth, h, w) of the stride-8 sparse output: cfg.sparse_shape through the four strided stages."""
    shape = cfg.sparse_shape
    for stage in STRIDED_STAGES:
        shape = ops.conv_out_shape(shape, *_DOWN[stage])
    return shape


# ---------------------------------------------------------------------------------------- layouts
def sparse_kio(w):
    """spconv-2.x weight (Cout, kD, kH, kW, Cin) -> [kv, Cin, Cout]"""
    return w.reshape(w.shape[0], -1, w.shape[-1]).permute(1, 2, 0)


def sparse_from_kio(w_kio, ksize):
    kv, c_in, c_out = w_kio.shape
    return w_kio.permute(2, 0, 1).reshape(c_out, ksize[0], ksize[1], ksize[2], c_in)


def conv2d_kio(w):
    """Conv2d weight (Cout, Cin, k, k) -> [k*k, Cin, Cout]"""
    return w.permute(2, 3, 1, 0).reshape(w.shape[2] * w.shape[3], w.shape[1], w.shape[0])


def conv2d_from_kio(w_kio, k):
    kv, c_in, c_out = w_kio.shape
    return w_kio.reshape(k, k, c_in, c_out).permute(3, 2, 0, 1)


def deconv_kio(w, u):
    """ConvTranspose2d(k = s = u) weight (Cin, Cout, u, u) -> [1, Cin, u*u*Cout]: one 1x1 GEMM with the u*u taps stacked along the columns"""
    return w.permute(0, 2, 3, 1).reshape(1, w.shape[0], u * u * w.shape[1])


def deconv_from_kio(w_kio, u, c_out):
    return w_kio.reshape(w_kio.shape[1], u, u, c_out).permute(0, 3, 1, 2)


def bev_first_conv_zc(w, C, depth):
    """input channels of the first BEV conv: the reference's c*D + z (height_compression.py:136-138) -> ours, z*C + c"""
    return w.reshape(w.shape[0], C, depth, *w.shape[2:]).permute(0, 2, 1, 3, 4).reshape(w.shape[0], depth * C, *w.shape[2:])


def bev_first_conv_from_zc(w, C, depth):
    return bev_first_conv_zc(w, depth, C)          # (the transposition of a C x depth block is undone by that of a depth x C one)


# ---------------------------------------------------------------------------------------- the layer walk
class LayerSpec(NamedTuple):
    conv: str                  # reference name of the conv module: its parameters are conv + ".weight" / ".bias"
    bn: Optional[str]          # ... of the BatchNorm behind it (None: the head's output convs)
    kind: str                  # "sparse" | "conv2d" | "deconv": the reference weight layout
    ksize: Tuple[int, ...]
    c_in: int                  # in the reference's layout (a deconv's c_out: before the u*u stacking)
    c_out: int
    mode: str                  # "same" | "strided" | "up" (train_engine._Conv)
    up: int
    group: str                 # whose BatchNorm constants: "sparse" | "bev" | "head"
    bias: bool                 # may the conv have a bias
    relu: bool
    first_bev: bool            # the conv that reads HeightCompression's channels (bev_first_conv_zc)
    slot: tuple                # where the layer goes: ("sparse", "conv_input" | "convN.down" | "conv_out"), ("sparse", "convN", block, 0 | 1),
    #                            ("bev", lvl, i), ("deblock", lvl), ("shared",), ("head", name, 0 | 1)

    def weight_shape(self):
        if self.kind == "sparse":
            return (self.c_out,) + self.ksize + (self.c_in,)
        return ((self.c_in, self.c_out) if self.kind == "deconv" else (self.c_out, self.c_in)) + self.ksize

    def kio(self, w, C, depth):
        """reference weight -> [kv, Cin, Cout] (C, depth: out_features and the final sparse depth, for the first BEV conv)"""
        if self.kind == "sparse":
            return sparse_kio(w)
        if self.kind == "deconv":
            return deconv_kio(w, self.up)
        return conv2d_kio(bev_first_conv_zc(w, C, depth) if self.first_bev else w)

    def from_kio(self, w_kio, C, depth):
        if self.kind == "sparse":
            return sparse_from_kio(w_kio, self.ksize)
        if self.kind == "deconv":
            return deconv_from_kio(w_kio, self.up, w_kio.shape[2] // (self.up * self.up))
        w = conv2d_from_kio(w_kio, self.ksize[0])
        return bev_first_conv_from_zc(w, C, depth) if self.first_bev else w


BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def centerpoint_layers(cfg, depth=None):
    """Every convolution of the one-stage CenterPoint graph, in the reference's module order. `depth`: z extent of the stride-8
    output (default final_shape(cfg)[0])."""
    if depth is None:
        depth = final_shape(cfg)[0]
    out = []

    def add(conv, bn, kind, ksize, c_in, c_out, slot, mode="same", up=1, group="sparse", bias=False, relu=True, first_bev=False):
        out.append(LayerSpec(conv, bn, kind, tuple(ksize), c_in, c_out, mode, up, group, bias, relu, first_bev, slot))

    nf = cfg.num_filters
    p = "backbone_3d."
    add(p + "conv_input.0", p + "conv_input.1", "sparse", [3, 3, 3], cfg.num_point_features, nf[0], ("sparse", "conv_input"))

    def basic_blocks(stage, first, c):               # two SparseBasicBlocks (spconv_backbone.py:120-136; relu of conv2: after the residual add)
        for b in range(2):
            name = p + "%s.%d" % (stage, first + b)
            for j in range(2):
                add(name + ".conv%d" % (j + 1), name + ".bn%d" % (j + 1), "sparse", [3, 3, 3], c, c, ("sparse", stage, b, j), bias=True)

    basic_blocks("conv1", 0, nf[0])
    for lvl, stage in enumerate(STRIDED_STAGES[:3], start=1):
        add(p + stage + ".0.0", p + stage + ".0.1", "sparse", _DOWN[stage][0], nf[lvl - 1], nf[lvl], ("sparse", stage + ".down"), mode="strided")
        basic_blocks(stage, 1, nf[lvl])
    add(p + "conv_out.0", p + "conv_out.1", "sparse", _DOWN["conv_out"][0], nf[3], cfg.out_features, ("sparse", "conv_out"), mode="strided")

    # BaseBEVBackbone (base_bev_backbone.py:27-59): ZeroPad2d, conv, BN, ReLU, then LAYER_NUMS x (conv, BN, ReLU)
    p = "backbone_2d."
    c_prev = cfg.out_features * depth
    for lvl, n in enumerate(cfg.bev_layer_nums):
        c = cfg.bev_num_filters[lvl]
        for i in range(n + 1):
            conv, bn = "blocks.%d.%d" % (lvl, 1 + 3 * i), "blocks.%d.%d" % (lvl, 2 + 3 * i)      # (0: the ZeroPad2d, 3 * i: the ReLUs)
            add(p + conv, p + bn, "conv2d", [3, 3], c_prev if i == 0 else c, c, ("bev", lvl, i), group="bev",
                mode="strided" if (i == 0 and cfg.bev_layer_strides[lvl] != 1) else "same", first_bev=(lvl == 0 and i == 0))
        u = cfg.bev_upsample_strides[lvl]
        add(p + "deblocks.%d.0" % lvl, p + "deblocks.%d.1" % lvl, "deconv", [u, u], c, cfg.bev_num_upsample_filters[lvl], ("deblock", lvl),
            mode="up", up=u, group="bev")
        c_prev = c

    # CenterHead (center_head.py:73-94, SeparateHead l.11-45; USE_BIAS_BEFORE_NORM True)
    p = "dense_head."
    sc = cfg.shared_conv_channel
    add(p + "shared_conv.0", p + "shared_conv.1", "conv2d", [3, 3], sum(cfg.bev_num_upsample_filters), sc, ("shared",), group="head", bias=True)
    for name in cfg.head_names():
        q = p + "heads_list.0.%s." % name
        add(q + "0.0", q + "0.1", "conv2d", [3, 3], sc, sc, ("head", name, 0), group="head", bias=True)
        add(q + "1", None, "conv2d", [3, 3], sc, cfg.head_out(name), ("head", name, 1), group="head", bias=True, relu=False)
    return out


def state_dict_names(layers):
    """the parameter and buffer names of a reference state_dict with these layers (without BatchNorm's num_batches_tracked)"""
    names = []
    for L in layers:
        names.append(L.conv + ".weight")
        if L.bias:
            names.append(L.conv + ".bias")
        if L.bn:
            names += [L.bn + "." + k for k in BN_KEYS]
    return names


def sparse_and_bev(cfg, at):
    """The containers the layer walks read, from `at` (slot -> layer object): sparse {"conv_input", "conv1": [(c1, c2), (c1, c2)],
    "conv2.down", "conv2", ..., "conv_out"} and bev_levels [(convs, deblock, u, c_up)]."""
    S = {"conv_input": at[("sparse", "conv_input")]}
    for stage in ("conv1",) + STRIDED_STAGES[:3]:
        if stage != "conv1":
            S[stage + ".down"] = at[("sparse", stage + ".down")]
        S[stage] = [(at[("sparse", stage, b, 0)], at[("sparse", stage, b, 1)]) for b in range(2)]
    S["conv_out"] = at[("sparse", "conv_out")]
    bev = []
    for lvl, n in enumerate(cfg.bev_layer_nums):
        de, u = at[("deblock", lvl)], cfg.bev_upsample_strides[lvl]
        bev.append(([at[("bev", lvl, i)] for i in range(n + 1)], de, u, de.c_out // (u * u)))
    return S, bev


def fuse_branches(first_w, first_scale, first_shift, last_w, last_bias):
    """Parallel two-conv branches on one input as two convs: the first convs side by side along Cout, the last convs block-diagonal.
    Lists of `[kv, Cin, Cout]` images (the first convs' with their folded scale / shift, the last convs' with their bias) ->
    (w1, s1, t1, w2, b2, slices), slices[i] = (first column, columns) of branch i in the fused output."""
    n_out = sum(w.shape[2] for w in last_w)
    w2 = torch.zeros(last_w[0].shape[0], sum(w.shape[1] for w in last_w), n_out)
    b2 = torch.zeros(n_out)
    slices = []
    row = col = 0
    for w, b in zip(last_w, last_bias):
        _, ci, co = w.shape
        w2[:, row:row + ci, col:col + co] = w
        b2[col:col + co] = b
        slices.append((col, co))
        row, col = row + ci, col + co
    return torch.cat(list(first_w), dim=2), torch.cat(list(first_scale)), torch.cat(list(first_shift)), w2, b2, slices


def split_branches_at(first_w, first_scale, first_shift, last_w, last_bias, keep):
    """The same parallel branches cut for a head that runs branch `keep` (CenterHead: the heat map) over every pixel and the others
    only where the decode reads them. -> dict: "keep1" (w, scale, shift) and "keep2" (w, bias) = branch `keep`'s own two convs (the
    columns it has in fuse_branches' w1 / s1 / t1; its block of w2); "rest1" (w, scale, shift) = the other branches' first convs side by
    side, in their order; "rest2" (w [kv, sum Cin, sum Cout], bias) = their last convs block-diagonal (zeros included), the fp32 image of
    cpd_center_decode_at_peaks; "rest_slices"[i] = (first column, columns) of the i-th other branch in it."""
    rest = [i for i in range(len(first_w)) if i != keep]
    pick = lambda xs: [xs[i] for i in rest]
    w1, s1, t1, w2, b2, slices = fuse_branches(pick(first_w), pick(first_scale), pick(first_shift), pick(last_w), pick(last_bias))
    return dict(keep1=(first_w[keep], first_scale[keep], first_shift[keep]), keep2=(last_w[keep], last_bias[keep]),
                rest1=(w1, s1, t1), rest2=(w2, b2), rest_slices=slices)
