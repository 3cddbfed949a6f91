"""RoI-head feature pooling of the two-stage CPD model on the C-ABI kernels of
csrc/roi_pool.hip. Mirrors, name for name:

  generate_voxel2pinds                        cpd/utils/spconv_utils.py:14-21
  voxel_query / VoxelQueryAndGrouping          cpd/ops/pointnet2/pointnet2_stack/voxel_query_utils.py:10-110
  grouping_operation                           cpd/ops/pointnet2/pointnet2_stack/pointnet2_utils.py:48-84
  NeighborVoxelSAModuleMSG                     cpd/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py:8-131
  get_global_grid_points_of_roi, roi_grid_pool cpd/models/roi_heads/voxel_rcnn_head.py:186-273, 365-386
  VoxelRCNNHead                                cpd/models/roi_heads/voxel_rcnn_head.py:664-913 (eval and training forward,
                                               RoIHeadTemplate.get_loss through the fused `cpd_rcnn_loss`)

In eval mode (BatchNorm folded) the per-voxel MLP (mlps_in) and the output MLP
(mlps_out) are 1x1 `cpd_gather_conv` GEMMs; grouping, position encoding, ReLU and max-pool are one
fused kernel (`cpd_voxel_pool_max`), so the (M, C, nsample) grouped tensors of the reference are
never materialised. In training mode the module follows the reference's sequence with the differentiable
`GroupingOperation` (`cpd_group_points` / `cpd_group_points_grad`); see cpd_amd/roi_head_train.py. With `fused_train` on, training
fuses the same span as well (`cpd_voxel_pool_moments` / `cpd_voxel_pool_max_train` / `cpd_voxel_pool_max_train_grad`): the
position branch is linear, so its batch statistics and BatchNorm backward come from the moments of the neighbour offsets. The neighbour query can use the sparse tensor's own site index
(`cpd_voxel_query_index`) instead of a dense (B,Z,Y,X) volume.
"""
import ctypes

import torch
import torch.nn as nn

from . import ops
from .autograd_ops import HipBatchNorm1d, HipBatchNorm2d, HipConv1d, HipLinear, HipPointwiseConv2d
from ._lib import check, iarr, lib, ptr, stream


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def cell_geometry(voxel_size, downsample_times, point_cloud_range):
    """(cell_xyz, origin_xyz) as two ctypes float[3]: the fp32 constants get_voxel_centers (common_utils.py:66-82) multiplies and adds
    with -- float32(voxel_size) * stride, float32(point_cloud_range[0:3]) -- for the queries that evaluate voxel centres from cell
    coordinates (`cpd_voxel_query_index_grid`)."""
    vs = (torch.tensor([float(v) for v in voxel_size]).float() * downsample_times).tolist()
    org = torch.tensor([float(v) for v in point_cloud_range[0:3]]).float().tolist()
    return (ctypes.c_float * 3)(*vs), (ctypes.c_float * 3)(*org)


def _query_index(index, nsample, radius, ranges, new_xyz, xyz, new_coords, idx, grid=None):
    """the bitmap-index query: from cell geometry (`grid` = cell_geometry(...), window rows of <= 32 cells) or from the xyz rows"""
    zr, yr, xr = [int(v) for v in ranges]
    z, y, x = index.shape
    m = new_coords.shape[0]
    if grid is not None and 2 * xr + 1 <= 32:
        check(lib().cpd_voxel_query_index_grid(m, index.batch, z, y, x, int(nsample), float(radius), zr, yr, xr, ptr(new_xyz), ptr(new_coords),
                                               ptr(index.buf), xyz.shape[0], grid[0], grid[1], ptr(idx), stream()), "cpd_voxel_query_index_grid")
    else:
        check(lib().cpd_voxel_query_index(m, index.batch, z, y, x, int(nsample), float(radius), zr, yr, xr, ptr(new_xyz), ptr(xyz),
                                          ptr(new_coords), ptr(index.buf), 0, xyz.shape[0], ptr(idx), stream()), "cpd_voxel_query_index")


def generate_voxel2pinds(indices, batch_size, spatial_shape):
    """indices [n,4] i32 (b,z,y,x) -> int32 (B,Z,Y,X) volume of row ids, -1 = empty."""
    indices = indices.contiguous()
    out = torch.empty([batch_size] + [int(s) for s in spatial_shape], dtype=torch.int32, device=indices.device)
    check(lib().cpd_voxel2pinds(ptr(indices), indices.shape[0], int(batch_size), iarr(spatial_shape), ptr(out), stream()),
          "cpd_voxel2pinds")
    return out


def voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices=None, index=None, grid=None):
    """VoxelQuery.forward: (idx [M, nsample] i32 with empty balls zeroed, empty_ball_mask [M] bool).
    new_coords [M,4] = (b,z,y,x). Pass `point_indices` (dense volume) like the reference, or `index`
    (an ops.SiteIndex of the sparse tensor; whether its ranks are row ids or go through its permutation is recorded in the
    index buffer itself and read on the device). `grid` = cell_geometry(...) with an index: xyz ARE the cells' centres
    (get_voxel_centers), and the kernel computes them instead of loading them."""
    idx = voxel_query_raw(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices, index, grid)
    empty = idx[:, 0] == -1
    idx[empty] = 0
    return idx, empty


def voxel_query_raw(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices=None, index=None, grid=None):
    """The query kernel's own output: idx [M, nsample] i32 of GLOBAL rows, idx[m, 0] == -1 for an empty ball (its other slots 0), the
    slots behind the last hit pre-filled with the first -- what the fused pooling kernels take."""
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and new_coords.is_contiguous()
    m = new_coords.shape[0]
    idx = torch.zeros((m, nsample), dtype=torch.int32, device=xyz.device)
    zr, yr, xr = [int(v) for v in max_range]
    if index is not None:
        _query_index(index, nsample, radius, max_range, new_xyz, xyz, new_coords, idx, grid)
    else:
        assert point_indices.is_contiguous() and point_indices.dtype == torch.int32
        b, z, y, x = point_indices.shape
        check(lib().cpd_voxel_query(m, z, y, x, int(nsample), float(radius), zr, yr, xr, ptr(new_xyz), ptr(xyz), ptr(new_coords),
                                    ptr(point_indices), ptr(idx), stream()), "cpd_voxel_query")
    return idx


def grouping_operation(features, features_batch_cnt, idx, idx_batch_cnt):
    """GroupingOperation.forward: (M, C, nsample) = features[batch start + idx]."""
    features, idx = features.contiguous(), idx.contiguous()
    m, ns = idx.shape
    c = features.shape[1]
    out = torch.empty((m, c, ns), dtype=torch.float32, device=features.device)
    check(lib().cpd_group_points(int(features_batch_cnt.shape[0]), m, c, ns, ptr(features), ptr(features_batch_cnt.int().contiguous()),
                                 ptr(idx), ptr(idx_batch_cnt.int().contiguous()), ptr(out), stream()), "cpd_group_points")
    return out


class GroupingOperation(torch.autograd.Function):
    """pointnet2_utils.GroupingOperation (pointnet2_utils.py:48-108): forward `cpd_group_points`, backward
    `cpd_group_points_grad` (the scatter-add of the grouped gradient back to the feature rows)."""

    @staticmethod
    def forward(ctx, features, features_batch_cnt, idx, idx_batch_cnt):
        out = grouping_operation(features, features_batch_cnt, idx, idx_batch_cnt)
        ctx.n = features.shape[0]
        ctx.save_for_backward(features_batch_cnt.int().contiguous(), idx.contiguous(), idx_batch_cnt.int().contiguous())
        return out

    @staticmethod
    def backward(ctx, grad_out):
        fcnt, idx, icnt = ctx.saved_tensors
        grad_out = grad_out.contiguous().float()
        m, c, ns = grad_out.shape
        g = torch.empty((ctx.n, c), dtype=torch.float32, device=grad_out.device)
        check(lib().cpd_group_points_grad(int(fcnt.shape[0]), m, c, ns, ctx.n, ptr(grad_out), ptr(fcnt), ptr(idx), ptr(icnt), ptr(g),
                                          stream()), "cpd_group_points_grad")
        return g, None, None, None


def voxel_query_and_grouping(max_range, radius, nsample, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features,
                             voxel2point_indices=None, index=None):
    """VoxelQueryAndGrouping.forward (voxel_query_utils.py:61-110): (grouped_features (M, C, ns), grouped_xyz (M, 3, ns),
    empty_ball_mask (M)); differentiable in `features`. The query returns global rows; they are made per-sample like the
    reference does before grouping."""
    idx, empty = voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, voxel2point_indices, index)
    batch = xyz_batch_cnt.shape[0]
    starts = torch.cumsum(xyz_batch_cnt.int(), 0) - xyz_batch_cnt.int()
    per_pt = torch.repeat_interleave(starts, new_xyz_batch_cnt.long()) if batch > 1 else None
    if per_pt is not None:
        idx = idx - per_pt[:, None].int()
    idx[empty] = 0
    grouped_xyz = GroupingOperation.apply(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
    grouped_features = GroupingOperation.apply(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
    return grouped_features, grouped_xyz, empty


def voxel_pool_max(features_in, xyz, new_xyz, idx_raw, w_pos, b_pos):
    """Fused grouping + position MLP + ReLU + max over samples -> [M, C]. idx_raw: kernel output
    (global rows, idx[m,0] == -1 for an empty ball)."""
    m, ns = idx_raw.shape
    c = features_in.shape[1]
    out = torch.empty((m, c), dtype=torch.float32, device=features_in.device)
    check(lib().cpd_voxel_pool_max(m, c, ns, _p(features_in), features_in.stride(0), ptr(xyz), ptr(new_xyz), ptr(idx_raw),
                                   ptr(w_pos), ptr(b_pos), _p(out), out.stride(0), stream()), "cpd_voxel_pool_max")
    return out


POOL_TRAIN_CHANNELS = (16, 32, 64)          # what cpd_voxel_pool_max_train (and the eval kernel) is instantiated for


def voxel_pool_max_train(features_in, xyz, new_xyz, idx_raw, w_pos, gamma, beta, running_mean, running_var, eps, momentum):
    """cpd_voxel_pool_moments + cpd_voxel_pool_max_train: grouping + position conv + BatchNorm2d on batch statistics + ReLU + max over
    the samples (voxel_pool_modules.py:96-117) without an (M, C, nsample) tensor. features_in [N, C] (rows may be strided), w_pos [C, 3],
    idx_raw as voxel_query_raw gives it; running_mean / running_var are updated in place. Returns (out [M, C], arg [M, C] uint8 = the
    sample attaining the maximum, 255 = cut off by the ReLU, mean [C], invstd [C], moments [9] float64)."""
    m, ns = idx_raw.shape
    c = features_in.shape[1]
    dev = features_in.device
    assert features_in.stride(1) == 1 and xyz.is_contiguous() and new_xyz.is_contiguous() and idx_raw.is_contiguous()
    assert w_pos.shape == (c, 3) and w_pos.is_contiguous() and gamma.is_contiguous() and beta.is_contiguous()
    ws = torch.empty(lib().cpd_voxel_pool_train_workspace_bytes(m, c, ns), dtype=torch.uint8, device=dev)
    moments = torch.empty(9, dtype=torch.float64, device=dev)
    check(lib().cpd_voxel_pool_moments(m, ns, xyz.shape[0], ptr(xyz), ptr(new_xyz), ptr(idx_raw), ptr(moments), ptr(ws), ws.numel(), stream()),
          "cpd_voxel_pool_moments")
    out = torch.empty((m, c), dtype=torch.float32, device=dev)
    arg = torch.empty((m, c), dtype=torch.uint8, device=dev)
    mean, invstd = torch.empty(c, dtype=torch.float32, device=dev), torch.empty(c, dtype=torch.float32, device=dev)
    check(lib().cpd_voxel_pool_max_train(m, c, ns, xyz.shape[0], _p(features_in), features_in.stride(0), ptr(xyz), ptr(new_xyz), ptr(idx_raw),
                                         ptr(w_pos), ptr(gamma), ptr(beta), ptr(moments), float(eps), float(momentum), _p(running_mean),
                                         _p(running_var), ptr(out), out.stride(0), ptr(arg), ptr(mean), ptr(invstd), stream()),
          "cpd_voxel_pool_max_train")
    return out, arg, mean, invstd, moments


def voxel_pool_max_train_grad(grad_out, arg, idx_raw, xyz, new_xyz, w_pos, gamma, mean, invstd, moments, eps, n_rows):
    """cpd_voxel_pool_max_train_grad -> (d features_in [n_rows, C] by float atomics, d w_pos [C, 3], d gamma [C], d beta [C]; the last
    three from float64 sums in a fixed order)."""
    m, ns = idx_raw.shape
    c = arg.shape[1]
    dev = arg.device
    assert grad_out.stride(1) == 1
    ws = torch.empty(lib().cpd_voxel_pool_train_workspace_bytes(m, c, ns), dtype=torch.uint8, device=dev)
    dfin = torch.empty((n_rows, c), dtype=torch.float32, device=dev)
    dw = torch.empty((c, 3), dtype=torch.float32, device=dev)
    dgamma, dbeta = torch.empty(c, dtype=torch.float32, device=dev), torch.empty(c, dtype=torch.float32, device=dev)
    check(lib().cpd_voxel_pool_max_train_grad(m, c, ns, n_rows, _p(grad_out), grad_out.stride(0), ptr(arg), ptr(idx_raw), ptr(xyz), ptr(new_xyz),
                                              ptr(w_pos), ptr(gamma), ptr(mean), ptr(invstd), ptr(moments), float(eps), _p(dfin), ptr(dw),
                                              ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), stream()), "cpd_voxel_pool_max_train_grad")
    return dfin, dw, dgamma, dbeta


class VoxelPoolMaxTrain(torch.autograd.Function):
    """The fused pooling of one scale in training (voxel_pool_max_train / voxel_pool_max_train_grad): differentiable in features_in and in
    the position branch's parameters (conv weight [C, 3, 1, 1], BatchNorm weight and bias); xyz / new_xyz get no gradient (the RoIs are
    detached). The running statistics are updated in place by the forward; num_batches_tracked is the caller's."""

    @staticmethod
    def forward(ctx, features_in, conv_weight, gamma, beta, xyz, new_xyz, idx_raw, running_mean, running_var, eps, momentum):
        fin = features_in.detach().float()
        if fin.stride(1) != 1:
            fin = fin.contiguous()
        c = fin.shape[1]
        w = conv_weight.detach().reshape(c, 3).contiguous().float()
        g, b = gamma.detach().contiguous().float(), beta.detach().contiguous().float()
        out, arg, mean, invstd, moments = voxel_pool_max_train(fin, xyz, new_xyz, idx_raw, w, g, b, running_mean, running_var, eps, momentum)
        ctx.save_for_backward(arg, idx_raw, xyz, new_xyz, w, g, mean, invstd, moments)
        ctx.eps, ctx.n_rows, ctx.w_shape = float(eps), fin.shape[0], conv_weight.shape
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        arg, idx_raw, xyz, new_xyz, w, g, mean, invstd, moments = ctx.saved_tensors
        grad_out = grad_out.float()
        if grad_out.stride(1) != 1:
            grad_out = grad_out.contiguous()
        dfin, dw, dgamma, dbeta = voxel_pool_max_train_grad(grad_out, arg, idx_raw, xyz, new_xyz, w, g, mean, invstd, moments, ctx.eps,
                                                            ctx.n_rows)
        return dfin, dw.view(ctx.w_shape), dgamma, dbeta, None, None, None, None, None, None, None


def set_fused_train(model, on=True):
    """Flip `fused_train` on every NeighborVoxelSAModuleMSG of `model` (both pooling stacks of VoxelRCNNProtoHead, VoxelRCNNHead's);
    returns how many there were."""
    n = 0
    for mod in model.modules():
        if isinstance(mod, NeighborVoxelSAModuleMSG):
            mod.fused_train = bool(on)
            n += 1
    return n


def _fold(bn):
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias.detach() - bn.running_mean * scale


class NeighborVoxelSAModuleMSG(nn.Module):
    """State-dict compatible with the reference module (mlps_in / mlps_pos / mlps_out). Eval mode: BatchNorm folded, three
    launches per scale (see the module docstring). Training mode: the reference's own sequence (voxel_pool_modules.py:86-128) --
    torch Conv / BatchNorm modules with batch statistics on the device, the neighbour query and the differentiable grouping
    (`GroupingOperation`) on the C-ABI kernels --, so gradients reach the MLPs and, through `features`, the sparse backbone.
    `fused_train` (default False; set_fused_train flips it on a whole model): training runs grouping + mlps_pos + ReLU + max-pool of a
    scale as ONE differentiable op (VoxelPoolMaxTrain) that stores no (M, C, nsample) tensor; parameters and state-dict are the same.
    A scale the fused kernels do not cover -- the cases in which HipBatchNorm2d itself leaves its kernel path (BatchNorm in eval mode,
    without running statistics, affine or momentum, a single slot), a width other than 16 / 32 / 64, coordinates that require a
    gradient -- takes the module sequence as before."""

    def __init__(self, *, query_ranges, radii, nsamples, mlps, use_xyz=True, pool_method="max_pool"):
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        if pool_method != "max_pool":
            raise NotImplementedError("only max_pool is used by the CPD configs (voxel_rcnn_cproto_center*.yaml POOL_METHOD)")
        self.query_ranges, self.radii, self.nsamples = query_ranges, radii, nsamples
        self.mlps_in, self.mlps_pos, self.mlps_out = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for spec in mlps:
            # (round 5: BatchNorm and the 3 -> C position conv on the C-ABI kernels too -- training runs no torch conv / BatchNorm kernel)
            self.mlps_in.append(nn.Sequential(HipConv1d(spec[0], spec[1], kernel_size=1, bias=False), HipBatchNorm1d(spec[1])))
            self.mlps_pos.append(nn.Sequential(HipPointwiseConv2d(3, spec[1], kernel_size=1, bias=False), HipBatchNorm2d(spec[1])))
            self.mlps_out.append(nn.Sequential(HipConv1d(spec[1], spec[2], kernel_size=1, bias=False), HipBatchNorm1d(spec[2]),
                                               nn.ReLU()))
        for m in self.modules():                                   # init_weights, voxel_pool_modules.py:60-68
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
        self._packed = None
        self.fused_train = False

    def _fused_scale(self, k, xyz, new_xyz):
        """whether scale k takes the fused training op (the conditions of autograd_ops._bn_rows' kernel path, and the kernels' own)"""
        conv, bn = self.mlps_pos[k][0], self.mlps_pos[k][1]
        return bool(self.fused_train and bn.training and bn.track_running_stats and bn.affine and bn.momentum is not None
                    and xyz.is_cuda and new_xyz.shape[0] * int(self.nsamples[k]) > 1 and int(self.nsamples[k]) <= 255
                    and conv.out_channels in POOL_TRAIN_CHANNELS and not xyz.requires_grad and not new_xyz.requires_grad)

    def fused_train_ready(self, xyz, new_xyz):
        """True when a training forward on these coordinates runs EVERY scale fused: the per-sample row counts are then not needed"""
        return self.training and all(self._fused_scale(k, xyz, new_xyz) for k in range(len(self.nsamples)))

    def _pack(self):
        pk = []
        for k in range(len(self.nsamples)):
            s_in, t_in = _fold(self.mlps_in[k][1])
            w_in = self.mlps_in[k][0].weight.detach()[:, :, 0].t().contiguous()[None]          # [1, C0, C1]
            s_p, t_p = _fold(self.mlps_pos[k][1])
            w_pos = (self.mlps_pos[k][0].weight.detach()[:, :, 0, 0] * s_p[:, None]).t().contiguous()   # [3, C1]
            s_o, t_o = _fold(self.mlps_out[k][1])
            w_out = self.mlps_out[k][0].weight.detach()[:, :, 0].t().contiguous()[None]        # [1, C1, C2]
            pk.append(dict(w_in=ops.pack_weight(w_in), s_in=s_in.contiguous(), t_in=t_in.contiguous(), w_pos=w_pos,
                           b_pos=t_p.contiguous(), w_out=ops.pack_weight(w_out), s_out=s_o.contiguous(), t_out=t_o.contiguous(),
                           w_out_folded=(w_out[0] * s_o[None, :]).contiguous(),                      # [C1, C2]: the fused pooling kernel's form
                           c0=w_in.shape[1], c1=w_in.shape[2], c2=w_out.shape[2]))
        self._packed = pk

    def _forward_train(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices, index):
        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()
        outs = []
        for k in range(len(self.nsamples)):
            fin = self.mlps_in[k](features.permute(1, 0).unsqueeze(0))                       # (1, C1, N)
            fin = fin.permute(0, 2, 1).contiguous().view(-1, fin.shape[1])                   # (N, C1)
            if self._fused_scale(k, xyz, new_xyz):
                conv, bn = self.mlps_pos[k][0], self.mlps_pos[k][1]
                idx = voxel_query_raw(self.query_ranges[k], self.radii[k], self.nsamples[k], xyz, new_xyz, new_coords, voxel2point_indices, index)
                x = VoxelPoolMaxTrain.apply(fin, conv.weight, bn.weight, bn.bias, xyz, new_xyz, idx, bn.running_mean, bn.running_var, bn.eps,
                                            bn.momentum)
                with torch.no_grad():
                    bn.num_batches_tracked += 1
                outs.append(self.mlps_out[k](x.t().unsqueeze(0)).squeeze(0).permute(1, 0))
                continue
            assert xyz_batch_cnt is not None, "the module sequence groups per sample: pass xyz_batch_cnt"
            gf, gx, empty = voxel_query_and_grouping(self.query_ranges[k], self.radii[k], self.nsamples[k], new_coords, xyz,
                                                     xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, fin, voxel2point_indices, index)
            keep = (~empty).to(gf.dtype)[:, None, None]
            gf = (gf * keep).permute(1, 0, 2).unsqueeze(0)                                   # zeroed empty balls, (1, C1, M, ns)
            gx = ((gx - new_xyz.unsqueeze(-1)) * keep).permute(1, 0, 2).unsqueeze(0)         # (1, 3, M, ns)
            x = torch.relu(gf + self.mlps_pos[k](gx))
            x = x.max(dim=3)[0]                                                              # max_pool2d over the samples
            outs.append(self.mlps_out[k](x).squeeze(0).permute(1, 0))
        return torch.cat(outs, dim=1)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices=None,
                index=None, grid=None, out=None, out_block=None):
        """`index` / `grid` / `out` (beyond the reference's arguments): the level's ops.SiteIndex instead of the dense volume, its
        cell_geometry(...) when xyz = get_voxel_centers of that level (eval: the query then computes the centres), and (eval) the
        [M, sum C2] block to write -- may be a column slice of wider rows."""
        if self.training:
            self._packed = None
            return self._forward_train(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices, index)
        with torch.no_grad():
            return self._forward_eval(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices, index, grid, out,
                                      out_block)

    def _forward_eval(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices, index, grid=None, out=None,
                      out_block=None):
        """`out_block` (eval): an absmax block (ops.absmax_blocks) the pooling kernels raise to max |out| of what they write -- the range
        block of the pooled rows for a split-fp16 consumer (cpd_voxel_pool_max_mlp_ranged)"""
        if self._packed is None:
            self._pack()
        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()                 # (b,x,y,z) -> (b,z,y,x), l.84
        n, m = features.shape[0], new_xyz.shape[0]
        width = sum(pk["c2"] for pk in self._packed)
        if out is None:
            out = torch.empty((m, width), dtype=torch.float32, device=xyz.device)
        assert out.shape == (m, width) and out.stride(1) == 1
        col = 0
        for k, pk in enumerate(self._packed):
            if isinstance(features, ops.PairRows):         # fp16-pair rows straight from the engine's sparse level: the split-fp16 row-wave GEMM
                fin = ops.gather_conv(features.rows, pk["c0"], pk["w_in"], None, 1, n, pk["c1"], pk["s_in"], pk["t_in"], None, False, math="f16x2",
                                      in_pairs=True)
            else:
                fin = ops.gather_conv(features, pk["c0"], pk["w_in"], None, 1, n, pk["c1"], pk["s_in"], pk["t_in"], None, False)
            idx = torch.zeros((m, self.nsamples[k]), dtype=torch.int32, device=xyz.device)
            zr, yr, xr = self.query_ranges[k]
            if index is not None:
                _query_index(index, self.nsamples[k], self.radii[k], (zr, yr, xr), new_xyz, xyz, new_coords, idx, grid)
            else:
                b, z, y, x = voxel2point_indices.shape
                check(lib().cpd_voxel_query(m, z, y, x, self.nsamples[k], float(self.radii[k]), zr, yr, xr, ptr(new_xyz), ptr(xyz),
                                            ptr(new_coords), ptr(voxel2point_indices), ptr(idx), stream()), "cpd_voxel_query")
            if pk["c1"] in (16, 32, 64) and pk["c2"] <= 2 * pk["c1"]:        # pooling + output MLP in one kernel, written straight into the scales' shared rows
                o = out[:, col:col + pk["c2"]]
                check(lib().cpd_voxel_pool_max_mlp_ranged(m, pk["c1"], self.nsamples[k], _p(fin), fin.stride(0), ptr(xyz), ptr(new_xyz), ptr(idx),
                                                          ptr(pk["w_pos"]), ptr(pk["b_pos"]), ptr(pk["w_out_folded"]), ptr(pk["t_out"]), pk["c2"], 1,
                                                          _p(o), out.stride(0), ptr(out_block), stream()), "cpd_voxel_pool_max_mlp")
            else:
                pooled = voxel_pool_max(fin, xyz, new_xyz, idx, pk["w_pos"], pk["b_pos"])
                out[:, col:col + pk["c2"]] = ops.gather_conv(pooled, pk["c1"], pk["w_out"], None, 1, m, pk["c2"], pk["s_out"], pk["t_out"], None, True)
                if out_block is not None:
                    ops.absmax_rows(out[:, col:col + pk["c2"]], block=out_block)
            col += pk["c2"]
        return out


def get_voxel_centers(voxel_coords_zyx, downsample_times, voxel_size, point_cloud_range):
    """common_utils.get_voxel_centers (cpd/utils/common_utils.py:66-82)."""
    centers = voxel_coords_zyx[:, [2, 1, 0]].float()
    vs = torch.tensor(voxel_size, device=centers.device).float() * downsample_times
    return (centers + 0.5) * vs + torch.tensor(point_cloud_range[0:3], device=centers.device).float()


_DENSE_IDX = {}


def get_global_grid_points_of_roi(rois, grid_size):
    """voxel_rcnn_head.py:365-386: (B*N, G^3, 3) global grid points of each RoI (torch on the device)."""
    rois = rois.view(-1, rois.shape[-1])
    # the (G^3, 3) index triples of the reference's `new_ones(G, G, G).nonzero()` (row-major), built once per (G, device): nonzero() reads its
    # count back to the host on every call; broadcast instead of .repeat(n, 1, 1) -- the same values through the same operations
    key = (int(grid_size), rois.device)
    dense_idx = _DENSE_IDX.get(key)
    if dense_idx is None:
        dense_idx = _DENSE_IDX[key] = rois.new_ones((grid_size, grid_size, grid_size)).nonzero().float()[None]
    size = rois[:, 3:6]
    local = (dense_idx + 0.5) / grid_size * size.unsqueeze(1) - size.unsqueeze(1) / 2
    # rotate_points_along_z (common_utils.py:35-57): local @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] written out -- two products and one sum
    # per coordinate, elementwise on the device. (torch.matmul here was a batched rocBLAS GEMM of 3 x 3 matrices: the one vendor-library
    # call left on the inference path, round 5)
    ca, sa = torch.cos(rois[:, 6])[:, None], torch.sin(rois[:, 6])[:, None]
    lx, ly = local[..., 0], local[..., 1]
    rotated = torch.stack((lx * ca - ly * sa, lx * sa + ly * ca, local[..., 2]), dim=-1)
    return rotated + rois[:, None, 0:3], local


def roi_grid_points(rois, grid_size, voxel_size, point_cloud_range, strides=(), bzyx=False):
    """(grid_xyz [B*N*G^3, 3], {stride: int32 [B*N*G^3, 4] cell coordinates}) of rois [B, N, 7]: get_global_grid_points_of_roi and
    roi_grid_pool's `cur_coords` arithmetic (voxel_rcnn_head.py:186-273, 365-386) in one launch (cpd_roi_grid_points). Coordinates
    come as (b, x, y, z) like the reference's, or (b, z, y, x) with bzyx (what the neighbour queries take)."""
    assert rois.dim() == 3 and rois.shape[-1] >= 7
    b, n = rois.shape[0], rois.shape[1]
    flat = rois.reshape(b * n, rois.shape[-1]).contiguous().float()
    m = b * n * grid_size ** 3
    grid_xyz = torch.empty((m, 3), dtype=torch.float32, device=rois.device)
    strides = [int(v) for v in strides]
    coords = [torch.empty((m, 4), dtype=torch.int32, device=rois.device) for _ in strides]
    ptrs = (ctypes.c_void_p * max(1, len(strides)))(*[c.data_ptr() for c in coords])
    from ._lib import farr
    check(lib().cpd_roi_grid_points(_p(flat), flat.stride(0), b * n, n, int(grid_size), farr([float(v) for v in voxel_size]),
                                    farr([float(v) for v in point_cloud_range[0:3]]), len(strides), iarr(strides) if strides else None, ptrs,
                                    int(bool(bzyx)), _p(grid_xyz), stream()), "cpd_roi_grid_points")
    return grid_xyz, dict(zip(strides, coords))


def roi_grid_pool(rois, levels, strides, pool_layers, grid_size, voxel_size, point_cloud_range, batch_size, indexes=None, out_block=None):
    """VoxelRCNNHead.roi_grid_pool (voxel_rcnn_head.py:186-273). `levels[name]` = (features, indices, shape) as
    returned by CenterPointEngine.backbone3d; `pool_layers[name]` a NeighborVoxelSAModuleMSG; `indexes[name]`
    an optional ops.SiteIndex of that level (otherwise the dense voxel2pinds volume is built).
    Returns (B*N, G^3, sum C)."""
    # the grid points and their (b, x, y, z) cells at every pooled level: one launch (round 5; the torch sequence of the reference --
    # get_global_grid_points_of_roi, three floor divisions, cat, int -- was ~25 launches over B*N*G^3 points)
    grid_flat, cells = roi_grid_points(rois.reshape(batch_size, -1, rois.shape[-1]), grid_size, voxel_size, point_cloud_range,
                                       strides=sorted({int(strides[name]) for name in pool_layers}))
    per_frame = grid_flat.shape[0] // batch_size
    new_cnt = torch.full((batch_size,), per_frame, dtype=torch.int32, device=rois.device)
    pooled = []
    # eval: the levels' blocks are written side by side into one [M, sum C] tensor by the pooling kernels themselves (no torch.cat)
    fused = not torch.is_grad_enabled() and all(not layer.training for layer in pool_layers.values())
    widths = [sum(int(seq[0].out_channels) for seq in layer.mlps_out) for layer in pool_layers.values()] if fused else []
    whole = torch.empty((grid_flat.shape[0], sum(widths)), dtype=torch.float32, device=rois.device) if fused else None
    col = 0
    for name, layer in pool_layers.items():
        feats, coords, shape = levels[name]
        if isinstance(feats, ops.PairRows):
            if not fused:                                # the training branch differentiates through fp32 rows
                feats = feats.float_rows()
        elif not feats.is_contiguous():
            feats = feats.contiguous()
        stride = strides[name]
        xyz = get_voxel_centers(coords[:, 1:4], stride, voxel_size, point_cloud_range).contiguous()
        # (per-sample row counts: the training branch's grouping needs them; the fused eval path and the fused training op take global
        # rows and do not -- and bincount reads back)
        cnt = None if fused or layer.fused_train_ready(xyz, grid_flat) else torch.bincount(coords[:, 0].long(), minlength=batch_size).int()
        cur = cells[int(stride)]
        index = indexes.get(name) if indexes else None
        v2p = None if index is not None else generate_voxel2pinds(coords, batch_size, shape)
        out = layer(xyz=xyz, xyz_batch_cnt=cnt, new_xyz=grid_flat, new_xyz_batch_cnt=new_cnt,
                    new_coords=cur, features=feats, voxel2point_indices=v2p, index=index,
                    grid=cell_geometry(voxel_size, stride, point_cloud_range) if index is not None else None,
                    **(dict(out=whole[:, col:col + widths[len(pooled)]], out_block=out_block) if fused else {}))
        if fused:
            col += widths[len(pooled)]
        pooled.append(out if fused else out.view(-1, grid_size ** 3, out.shape[-1]))
    if fused:
        return whole.view(-1, grid_size ** 3, whole.shape[-1])
    return torch.cat(pooled, dim=-1)


def proposal_layer(batch_box_preds, batch_cls_preds, nms_thresh, nms_pre_maxsize, nms_post_maxsize, first_rows=None, device_fallback=False):
    """RoIHeadTemplate.proposal_layer (cpd/models/roi_heads/roi_head_template.py:53-114) for dense
    (B, N, 7+C) / (B, N, num_class) predictions with class-agnostic rotated NMS
    (model_nms_utils.class_agnostic_nms, l.115-134): per sample max class score -> top NMS_PRE_MAXSIZE ->
    rotated NMS -> first NMS_POST_MAXSIZE. All samples go through ONE batched mask / scan / select launch set
    (cpd_nms_batch, cpd_select_boxes); nothing is read back. Returns (rois [B, post, 7+C], roi_scores [B, post],
    roi_labels [B, post] i64 = argmax class + 1); slots past a sample's kept count are zero like the reference's
    new_zeros buffers (their label is 1: the reference's `roi_labels + 1` applies to every slot).
    `first_rows` = R (engines; round 5): only the first NMS_POST_MAXSIZE survivors are kept, and greedy suppression decides a box from the
    boxes before it -- the NMS runs over each sample's first R candidates (ops.nms_batch_first: R^2 / 2 IoUs instead of 4096^2 / 2, the
    scan stops at the NMS_POST_MAXSIZE-th survivor) and a fifth value comes back, `incomplete` [B] i32: 1 where a sample found fewer than
    NMS_POST_MAXSIZE survivors among its first R -- the caller reads it with the counts and calls again without `first_rows`.
    `device_fallback=True` (callers without a read-back: the module path): the full NMS of exactly those samples is queued right behind
    (ops.nms_batch_where, predicated on the device word) and four values come back as without `first_rows` -- the same answer as the
    full call, at the cost of a launch of empty workgroups when no sample needs it. `first_rows="auto"` = max(512, 4 x NMS_POST_MAXSIZE)."""
    if first_rows == "auto":
        first_rows = max(512, 64 * ((4 * int(nms_post_maxsize) + 63) // 64))
    b, n, cdim = batch_box_preds.shape
    scores, labels = torch.max(batch_cls_preds, dim=-1)                       # l.94
    k = min(int(nms_pre_maxsize), n)
    top_scores, order = torch.topk(scores, k=k, dim=1)                        # class_agnostic_nms l.124 (sorted descending)
    boxes = torch.gather(batch_box_preds, 1, order.unsqueeze(-1).expand(-1, -1, cdim)).contiguous()
    counts = torch.full((b,), k, dtype=torch.int32, device=boxes.device)
    incomplete = None
    if first_rows is not None and int(first_rows) < k:
        b7 = boxes[:, :, :7].contiguous()
        keep, num_keep, incomplete = ops.nms_batch_first(b7, counts, nms_thresh, int(nms_post_maxsize), int(first_rows))
        if device_fallback:
            ops.nms_batch_where(b7, counts, incomplete, nms_thresh, keep, num_keep)
    else:
        keep, num_keep = ops.nms_batch(boxes[:, :, :7].contiguous(), counts, nms_thresh)
    top_labels = torch.gather(labels, 1, order).int().contiguous()
    rois7, roi_scores, roi_labels, kept = ops.select_boxes(boxes[:, :, :7].contiguous(), top_scores.contiguous(), top_labels, keep,
                                                           num_keep, int(nms_post_maxsize), label_offset=1)
    valid = torch.arange(int(nms_post_maxsize), device=boxes.device)[None, :] < kept[:, None]
    # zero slots past a sample's count by SELECTION: cpd_select_boxes never wrote them (stale allocator bytes, possibly NaN bit patterns,
    # and NaN * 0 is NaN -- the hazard ADVICE r4 found in two_stage.py)
    rois7 = torch.where(valid[..., None], rois7, rois7.new_zeros(()))
    roi_scores = torch.where(valid, roi_scores, roi_scores.new_zeros(()))
    # the reference adds 1 to EVERY slot of its zero-initialised buffer (roi_head_template.py:111): padded slots carry label 1
    roi_labels = torch.where(valid, roi_labels, torch.ones_like(roi_labels))
    if cdim > 7:
        raise NotImplementedError("7+C box codes (velocity ...) are not used by the CPD configs")
    if first_rows is not None and not device_fallback:
        return rois7, roi_scores, roi_labels, kept, (incomplete if incomplete is not None else torch.zeros_like(kept))
    return rois7, roi_scores, roi_labels, kept


class VoxelRCNNHead(nn.Module):
    """VoxelRCNNHead (cpd/models/roi_heads/voxel_rcnn_head.py:664-763, 876-916), the RoI head of the anchor-head configs
    (voxel_rcnn_dbscan / oyster_single_train.yaml). Same constructor arguments and state_dict names as the reference module.

    Eval: RoI grid pooling, shared FC / cls / reg stacks (Linear + eval BatchNorm1d + ReLU folded into `cpd_gather_conv` GEMM
    epilogues) and RoIHeadTemplate.generate_predicted_boxes (roi_head_template.py:269-299), under no_grad.
    Training: proposal layer at NMS_CONFIG.TRAIN, proposal-target sampling and canonical targets (roi_head_train.assign_targets),
    the differentiable pooling path, the FC stacks as modules (batch-statistics BatchNorm, dropout) -> forward_ret_dict;
    get_loss() is RoIHeadTemplate.get_loss in one fused loss-and-gradient launch (`cpd_rcnn_loss`, roi_head_train.rcnn_head_loss).
    The constructor keeps torch's default initialisation of the FC stacks; init_weights() is the reference's (its constructor calls
    it): call it before training from scratch."""

    def __init__(self, input_channels, model_cfg, point_cloud_range=None, voxel_size=None, num_frames=1, num_class=1, **kwargs):
        super().__init__()
        self.model_cfg, self.point_cloud_range, self.voxel_size, self.num_class = model_cfg, point_cloud_range, voxel_size, num_class
        pool = model_cfg["ROI_GRID_POOL"]
        self.grid_size = pool["GRID_SIZE"]
        self.sources = list(pool["FEATURES_SOURCE"])
        self.roi_grid_pool_layers = nn.ModuleList()
        c_out = 0
        for src in self.sources:
            lc = pool["POOL_LAYERS"][src]
            mlps = [[input_channels[src]] + list(m) for m in lc["MLPS"]]
            self.roi_grid_pool_layers.append(NeighborVoxelSAModuleMSG(query_ranges=lc["QUERY_RANGES"], nsamples=lc["NSAMPLE"],
                                                                      radii=lc["POOL_RADIUS"], mlps=mlps, pool_method=lc["POOL_METHOD"]))
            c_out += sum(m[-1] for m in mlps)
        dp = model_cfg["DP_RATIO"]

        def stack(pre, widths, final=None):
            layers = []
            for k, wdt in enumerate(widths):
                layers += [HipLinear(pre, wdt, bias=False), HipBatchNorm1d(wdt), nn.ReLU()]
                pre = wdt
                if k != len(widths) - 1 and dp > 0:
                    layers.append(nn.Dropout(dp))
            if final is not None:
                layers.append(HipLinear(pre, final, bias=True))
            return nn.Sequential(*layers)

        self.shared_fc_layers = stack(self.grid_size ** 3 * c_out, model_cfg["SHARED_FC"])
        self.cls_layers = stack(model_cfg["SHARED_FC"][-1], model_cfg["CLS_FC"], num_class)
        self.reg_layers = stack(model_cfg["SHARED_FC"][-1], model_cfg["REG_FC"], 7 * num_class)
        self._fc = None
        # the training pieces (roi_head_template.py:15-28); an eval-only config may leave TARGET_CONFIG / LOSS_CONFIG out
        from .roi_head_train import ProposalTargetLayer
        tc, lc = model_cfg.get("TARGET_CONFIG"), model_cfg.get("LOSS_CONFIG")
        self.proposal_target_layer = ProposalTargetLayer(tc) if tc is not None else None
        if lc is not None:
            self.register_buffer("code_weights", torch.tensor(lc["LOSS_WEIGHTS"]["code_weights"], dtype=torch.float32), persistent=False)
        self.forward_ret_dict = {}

    def init_weights(self):
        """voxel_rcnn_head.py:747-763: xavier-normal on every Linear of the cls / reg stacks (bias 0), N(0, 0.01) on their output
        layers, then xavier-normal on the shared stack -- in that order, so that equal seeds give the reference's weights."""
        for stack in (self.cls_layers, self.reg_layers):
            for m in stack.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_normal_(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        for stack in (self.cls_layers, self.reg_layers):
            nn.init.normal_(stack[-1].weight, 0, 0.01)
            nn.init.constant_(stack[-1].bias, 0)
        for m in self.shared_fc_layers.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self._fc = None

    def _pack_fc(self):
        def pack(seq):
            out, mods, i = [], list(seq), 0
            while i < len(mods):
                lin = mods[i]
                if not isinstance(lin, nn.Linear):
                    i += 1
                    continue
                w = ops.pack_weight(lin.weight.detach().t().contiguous()[None])                # [1, in, out]
                if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d):
                    s, t = _fold(mods[i + 1])
                    out.append((w, lin.in_features, lin.out_features, s.contiguous(), t.contiguous(), True))
                else:
                    out.append((w, lin.in_features, lin.out_features, None, lin.bias.detach().contiguous(), False))
                i += 1
            return out
        self._fc = {k: pack(getattr(self, k)) for k in ("shared_fc_layers", "cls_layers", "reg_layers")}

    @staticmethod
    def _run(layers, x, math=None, in_block=None, return_block=False):
        """the stack as 1 x 1 GEMM launches. math = "f16x2": the split-fp16 tile kernels, range-guarded the whole way -- every layer
        takes the absmax block its producer filled (`in_block` for the first; measured when None) and fills the next one.
        return_block: also return the absmax block of the stack's output (None on the fp32 path), so that a caller feeding the output
        to further stacks does not measure it again."""
        if math != "f16x2":
            for w, cin, cout, s, t, relu in layers:
                x = ops.gather_conv(x, cin, w, None, 1, x.shape[0], cout, s, t, None, relu)
            return (x, None) if return_block else x
        blocks = ops.absmax_blocks(len(layers), x.device)
        rb = in_block if in_block is not None else ops.absmax_rows(x)
        for i, (w, cin, cout, s, t, relu) in enumerate(layers):
            ok = cin % 32 == 0 and cout % 64 == 0            # (the 256 -> 1 / 256 -> 7 output layers stay on the fp32 pipe)
            x = ops.gather_conv(x, cin, w, None, 1, x.shape[0], cout, s, t, None, relu, dense=True, math="f16x2" if ok else "f32",
                                in_absmax=rb if ok else None, out_absmax=blocks[i])
            rb = blocks[i]
        return (x, rb) if return_block else x

    def _proposals(self, batch_dict, mode):
        """RoIHeadTemplate.proposal_layer on the dense head's predictions (voxel_rcnn_head.py:883-885, roi_head_template.py:53-114):
        the anchor-head configs (voxel_rcnn_dbscan / oyster) reach the RoI head this way; CenterHead already left `rois` behind."""
        if "rois" in batch_dict:
            return
        nms = self.model_cfg["NMS_CONFIG"][mode]
        with torch.no_grad():
            rois7, roi_scores, roi_labels, _ = proposal_layer(batch_dict["batch_box_preds"], batch_dict["batch_cls_preds"], float(nms["NMS_THRESH"]),
                                                              int(nms["NMS_PRE_MAXSIZE"]), int(nms["NMS_POST_MAXSIZE"]),
                                                              first_rows="auto", device_fallback=True)
        batch_dict.update(rois=rois7, roi_scores=roi_scores, roi_labels=roi_labels,
                          has_class_labels=batch_dict["batch_cls_preds"].shape[-1] > 1)

    def _pool(self, batch_dict):
        levels = {}
        for name in self.sources:
            t = batch_dict["multi_scale_3d_features"][name]
            levels[name] = t if isinstance(t, tuple) else (t.features, t.indices, list(t.spatial_shape))
        return roi_grid_pool(batch_dict["rois"], levels, batch_dict["multi_scale_3d_strides"], dict(zip(self.sources, self.roi_grid_pool_layers)),
                             self.grid_size, self.voxel_size, self.point_cloud_range, batch_dict["batch_size"])

    def forward(self, batch_dict):
        if not self.training:
            return self._forward_eval(batch_dict)
        # training (voxel_rcnn_head.py:876-913): the packed eval FC images go stale with the first optimizer step
        self._fc = None
        from .roi_head_train import assign_targets
        self._proposals(batch_dict, "TRAIN")
        targets = assign_targets(self.proposal_target_layer, batch_dict)
        batch_dict["rois"], batch_dict["roi_labels"] = targets["rois"], targets["roi_labels"]
        pooled = self._pool(batch_dict)
        shared = self.shared_fc_layers(pooled.reshape(pooled.shape[0], -1))
        targets.update(rcnn_cls=self.cls_layers(shared), rcnn_reg=self.reg_layers(shared))
        self.forward_ret_dict = targets
        return batch_dict

    def get_loss(self, tb_dict=None):
        """RoIHeadTemplate.get_loss (roi_head_template.py:148-267) -> (rcnn_loss, tb_dict): one `cpd_rcnn_loss` launch for the loss and
        its gradient, one read-back of the loss vector for tb_dict (rcnn_loss_cls, rcnn_loss_reg = the smooth-L1 part,
        rcnn_loss_corner when the corner term is present, rcnn_loss)."""
        from .roi_head_train import rcnn_head_loss
        tb_dict = {} if tb_dict is None else tb_dict
        lc = self.model_cfg["LOSS_CONFIG"]
        if lc["CLS_LOSS"] != "BinaryCrossEntropy":
            raise NotImplementedError(lc["CLS_LOSS"])
        if lc["REG_LOSS"] != "smooth-l1":
            raise NotImplementedError(lc["REG_LOSS"])
        lw, t = lc["LOSS_WEIGHTS"], self.forward_ret_dict
        corner = bool(lc["CORNER_LOSS_REGULARIZATION"])
        loss, losses = rcnn_head_loss(t["rcnn_cls"], t["rcnn_reg"], t["rois"], t["gt_of_rois"], t["gt_of_rois_src"], t["reg_valid_mask"],
                                      t["rcnn_cls_labels"], lw["code_weights"], lw["rcnn_cls_weight"], lw["rcnn_reg_weight"],
                                      lw["rcnn_corner_weight"], corner)
        total, cls, reg, corner_loss, _bb, fg = losses.tolist()
        tb_dict.update(rcnn_loss_cls=cls, rcnn_loss_reg=reg)
        if corner and fg > 0:
            tb_dict["rcnn_loss_corner"] = corner_loss
        tb_dict["rcnn_loss"] = total
        return loss, tb_dict

    @torch.no_grad()
    def _forward_eval(self, batch_dict):
        if self._fc is None:
            self._pack_fc()
        self._proposals(batch_dict, "TEST")
        rois, b = batch_dict["rois"], batch_dict["batch_size"]
        pooled = self._pool(batch_dict)
        x = pooled.reshape(pooled.shape[0], -1).contiguous()
        shared = self._run(self._fc["shared_fc_layers"], x)
        rcnn_cls = self._run(self._fc["cls_layers"], shared)
        rcnn_reg = self._run(self._fc["reg_layers"], shared)
        cls, boxes = self.generate_predicted_boxes(b, rois, rcnn_cls, rcnn_reg)
        batch_dict.update(batch_box_preds=boxes, batch_cls_preds=cls, cls_preds_normalized=False)
        return batch_dict

    @staticmethod
    def generate_predicted_boxes(batch_size, rois, cls_preds, box_preds):
        """roi_head_template.py:269-299: decode the residuals against the RoI with its centre at the origin
        (cpd_anchor_decode), rotate by the RoI heading, translate to the RoI centre."""
        from . import anchor_head
        flat = rois.reshape(-1, rois.shape[-1])[:, :7].contiguous().float()
        local = flat.clone()
        local[:, 0:3] = 0
        n = flat.shape[0]
        _, dec = anchor_head.generate_predicted_boxes(local, 1, cls_preds.reshape(1, n, -1), box_preds.reshape(1, n, 7))
        dec = dec.view(n, 7)
        ca, sa = torch.cos(flat[:, 6]), torch.sin(flat[:, 6])
        x = dec[:, 0] * ca - dec[:, 1] * sa                          # rotate_points_along_z (common_utils.py:35-57)
        y = dec[:, 0] * sa + dec[:, 1] * ca
        out = torch.cat([(x + flat[:, 0])[:, None], (y + flat[:, 1])[:, None], (dec[:, 2] + flat[:, 2])[:, None], dec[:, 3:]], dim=1)
        return cls_preds.view(batch_size, -1, cls_preds.shape[-1]), out.view(batch_size, -1, 7)
