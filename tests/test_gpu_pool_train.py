"""GPU: the fused, differentiable RoI grid pooling for training (cpd_voxel_pool_moments / cpd_voxel_pool_max_train /
cpd_voxel_pool_max_train_grad, roi_pool.VoxelPoolMaxTrain, NeighborVoxelSAModuleMSG.fused_train) against the float64 restatement of
the reference sequence (tests/ref_pool_train.py; voxel_pool_modules.py:96-117), against the un-fused module sequence on the GPU, and
end to end against the two head-training fixtures.

Tolerances are those of tests/test_gpu_autograd.py::test_hip_batchnorm_and_pointwise_conv_match_torch: outputs atol 2e-5, running mean
atol 1e-6, running var rtol 1e-5 / atol 1e-6, d features / d gamma / d beta 2e-5 * max(scale, 1), d weight rtol 1e-4 / atol 1e-4.
A cell whose best and second-best candidates come from different rows and lie within 1e-5 of each other in the restatement may route
its gradient elsewhere in fp32: such cells carry no gradient in the comparison (at most 1 % of the cells; the share is asserted)."""
import copy
import functools

import numpy as np
import pytest
import torch

import ref_pool_train as R

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
# the forward / backward kernels walk 8 x (256 / C) points per block: 128 / 64 / 32 points at C = 16 / 32 / 64 -- M crosses each by one
SHAPES = [(m, ns, c) for m in (1, 33, 65, 129, 257) for ns in (1, 16) for c in (16, 32, 64) if m * ns > 1]


@functools.lru_cache(maxsize=None)
def _reference(m, ns, c, empty, dup, seed):
    """(case, float64 restatement results) -- computed once per case on the CPU and shared"""
    case = R.make_case(m, ns, c, n=50, seed=seed, empty=empty, dup=dup)
    case["beta"][3] = -50.0                                           # a channel whose maximum is <= 0 everywhere
    d = {k: case[k].double() for k in ("fin", "xyz", "new_xyz", "w", "gamma", "beta", "grad")}
    leaves = [d[k].clone().requires_grad_(True) for k in ("fin", "w", "gamma", "beta")]
    out, x, mean, var = R.restatement(leaves[0], d["xyz"], d["new_xyz"], case["idx"], leaves[1], leaves[2], leaves[3], EPS)
    tie = R.near_tie_cells(x.detach(), case["idx"]) & (out.detach() > 0)
    grad = torch.where(tie, torch.zeros_like(d["grad"]), d["grad"])   # near-tie cells are left out of the gradient comparison
    out.backward(grad)
    cf = R.closed_form(d["fin"], d["xyz"], d["new_xyz"], case["idx"], d["w"], d["gamma"], d["beta"], grad, EPS)
    rm, rv = R.running_update(case["running_mean"].double(), case["running_var"].double(), mean.detach(), var.detach(), m * ns, MOMENTUM)
    return case, dict(out=out.detach(), tie=tie, grad=grad, arg=cf["arg"], dfin=leaves[0].grad, dw=leaves[1].grad, dgamma=leaves[2].grad,
                      dbeta=leaves[3].grad, running_mean=rm, running_var=rv)


def _run_fused(case, grad, strided):
    from cpd_amd import roi_pool as rp
    c = case["fin"].shape[1]
    if strided:                                                       # rows of a wider tensor: features_ld > C
        wide = torch.zeros(case["fin"].shape[0], c + 12).cuda()
        wide[:, 4:4 + c] = case["fin"].cuda()
        fin = wide[:, 4:4 + c]
    else:
        fin = case["fin"].cuda()
    xyz, new_xyz, idx = case["xyz"].cuda(), case["new_xyz"].cuda(), case["idx"].cuda()
    w, gamma, beta = case["w"].cuda().contiguous(), case["gamma"].cuda(), case["beta"].cuda()
    rm, rv = case["running_mean"].cuda().clone(), case["running_var"].cuda().clone()
    out, arg, mean, invstd, moments = rp.voxel_pool_max_train(fin, xyz, new_xyz, idx, w, gamma, beta, rm, rv, EPS, MOMENTUM)
    dfin, dw, dgamma, dbeta = rp.voxel_pool_max_train_grad(grad.float().cuda(), arg, idx, xyz, new_xyz, w, gamma, mean, invstd, moments, EPS,
                                                           fin.shape[0])
    return dict(out=out, arg=arg, dfin=dfin, dw=dw, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv)


def _within(got, want, factor, what):
    got, want = got.detach().double().cpu(), want.double()
    scale = max(float(want.abs().max()), 1.0) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    print("%s: max |diff| %.3e, scale %.3e" % (what, err, scale))
    assert err <= factor * scale, what


def _check(m, ns, c, empty, dup, seed, strided):
    from cpd_amd import ops
    case, ref = _reference(m, ns, c, empty, dup, seed)
    share = float(ref["tie"].double().mean())
    print("near-tie cells: %d of %d" % (int(ref["tie"].sum()), ref["tie"].numel()))
    assert share <= 0.01
    with ops.launch_log() as log:
        got = _run_fused(case, ref["grad"], strided)
    assert log.counts == {"voxel_pool_moments_kernel": 1, "voxel_pool_max_train_kernel": 1, "voxel_pool_max_train_grad_kernel": 1}, log.counts
    err = float((got["out"].double().cpu() - ref["out"]).abs().max())
    print("out: max |diff| %.3e" % err)
    assert err <= 2e-5
    # the argmax away from ties and from the ReLU's threshold; the cut-off channel
    sure = ~ref["tie"] & ((ref["out"] > 1e-5) | (ref["arg"] == 255))
    zero_edge = (ref["arg"] == 255) & (got["arg"].cpu() != 255)      # a pre-activation within rounding of 0: not decidable in fp32
    assert int(zero_edge.sum()) <= 1
    assert torch.equal(got["arg"].cpu().long()[sure & ~zero_edge], ref["arg"][sure & ~zero_edge])
    assert bool((got["arg"][:, 3] == 255).all()) and float(got["out"][:, 3].abs().max()) == 0.0
    np.testing.assert_allclose(got["running_mean"].cpu().numpy(), ref["running_mean"].numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(got["running_var"].cpu().numpy(), ref["running_var"].numpy(), rtol=1e-5, atol=1e-6)
    for k in ("dfin", "dgamma", "dbeta"):
        _within(got[k], ref[k], 2e-5, k)
    np.testing.assert_allclose(got["dw"].double().cpu().numpy(), ref["dw"].numpy(), rtol=1e-4, atol=1e-4)
    if empty >= 1.0:
        assert float(got["dfin"].abs().max()) == 0.0
    # a second identical call: bitwise equal (the float64 sums run in a fixed order; only d features uses atomics)
    again = _run_fused(case, ref["grad"], strided)
    for k in ("out", "arg", "dw", "dgamma", "dbeta", "running_mean", "running_var"):
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("m,ns,c", SHAPES)
def test_fused_pool_matches_restatement(hip, m, ns, c):
    """about 15 % empty balls, duplicate pre-filled slots, 50 feature rows of two frames, strided feature rows"""
    _check(m, ns, c, 0.15, True, 100 + m + ns + c, strided=True)


@pytest.mark.parametrize("empty,dup", [(1.0, True), (0.0, False), (0.0, True)])
def test_fused_pool_with_all_or_no_balls_empty(hip, empty, dup):
    _check(257, 16, 32, empty, dup, 7, strided=False)


def test_entry_points_reject_what_they_do_not_cover(hip):
    from cpd_amd import roi_pool as rp
    from cpd_amd._lib import lib, ptr, stream
    case, _ = _reference(33, 16, 32, 0.15, True, 100 + 33 + 16 + 32)
    idx, xyz, new_xyz = case["idx"].cuda(), case["xyz"].cuda(), case["new_xyz"].cuda()
    f = torch.zeros(50, 64).cuda()
    z = torch.zeros(64).cuda()
    mom = torch.zeros(9, dtype=torch.float64).cuda()
    arg = torch.zeros(33, 64, dtype=torch.uint8).cuda()

    def fwd(m, c, ns):
        return lib().cpd_voxel_pool_max_train(m, c, ns, 50, ptr(f), 64, ptr(xyz), ptr(new_xyz), ptr(idx), ptr(f), ptr(z), ptr(z), ptr(mom), EPS,
                                              MOMENTUM, None, None, ptr(f), 64, ptr(arg), ptr(z), ptr(z), stream())
    assert fwd(33, 48, 16) == -4 and fwd(33, 8, 16) == -4            # CPD_ERR_UNSUPPORTED: C is 16, 32 or 64
    assert fwd(1, 32, 1) == -1 and fwd(0, 32, 16) == -1              # CPD_ERR_ARG: no batch statistics over <= 1 slot
    assert lib().cpd_voxel_pool_moments(33, 16, 50, ptr(xyz), ptr(new_xyz), ptr(idx), ptr(mom), ptr(f), 8, stream()) == -2   # workspace
    # rows outside [0, n_rows) are guarded: with n_rows = 25 the second frame's rows count as empty slots, nothing is read or written there
    out, arg2, mean, invstd, moments = rp.voxel_pool_max_train(case["fin"][:25].cuda(), xyz[:25].contiguous(), new_xyz, idx, case["w"].cuda(),
                                                               case["gamma"].cuda(), case["beta"].cuda(), None, None, EPS, MOMENTUM)
    dfin, dw, _, _ = rp.voxel_pool_max_train_grad(case["grad"].cuda(), arg2, idx, xyz[:25].contiguous(), new_xyz, case["w"].cuda(), case["gamma"].cuda(),
                                                  mean, invstd, moments, EPS, 25)
    assert dfin.shape == (25, 32) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(dfin).all()) and bool(torch.isfinite(dw).all())


# ---------------------------------------------------------------------------------------------------------------- the module
def _scene(seed=3, m_per=65, c0=8):
    """two frames of a (4, 16, 16) grid at 10 % occupancy, 1 m cells; grid points uniform over the range"""
    from cpd_amd import roi_pool as rp
    g = torch.Generator().manual_seed(seed)
    shape, vs, pcr = [4, 16, 16], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 16.0, 16.0, 4.0]
    coords = []
    for b in range(2):
        cells = torch.randperm(4 * 16 * 16, generator=g)[:100 + 7 * b].sort()[0]
        coords.append(torch.stack([torch.full_like(cells, b), cells // 256, (cells // 16) % 16, cells % 16], 1))
    coords = torch.cat(coords).int().cuda()
    feats = torch.randn(coords.shape[0], c0, generator=g).cuda()
    new_xyz = (torch.rand(2 * m_per, 3, generator=g) * torch.tensor([16.0, 16.0, 4.0])).cuda().contiguous()
    frame = torch.arange(2 * m_per).cuda() // m_per
    new_coords = torch.cat([frame[:, None].float(), torch.floor(new_xyz)], 1).int().contiguous()          # (b, x, y, z)
    xyz = rp.get_voxel_centers(coords[:, 1:4], 1, vs, pcr).contiguous()
    return dict(xyz=xyz, xyz_batch_cnt=torch.bincount(coords[:, 0].long(), minlength=2).int(), new_xyz=new_xyz,
                new_xyz_batch_cnt=torch.full((2,), m_per, dtype=torch.int32).cuda(), new_coords=new_coords, features=feats,
                voxel2point_indices=rp.generate_voxel2pinds(coords, 2, shape))


def _module(mlps, seed=5):
    from cpd_amd import roi_pool as rp
    torch.manual_seed(seed)
    mod = rp.NeighborVoxelSAModuleMSG(query_ranges=[[1, 1, 1], [2, 2, 2]][:len(mlps)], radii=[1.2, 2.4][:len(mlps)], nsamples=[8, 16][:len(mlps)],
                                      mlps=mlps)
    with torch.no_grad():
        for seq in mod.mlps_pos:
            seq[1].weight.uniform_(0.5, 1.5)
            seq[1].bias.normal_(0, 0.3)
    return mod.cuda().train()


def _run_module(mod, scene, grads, new_xyz_grad=False, counts=True):
    """forward + backward of sum_k <pooled_k, grads[k]> with the pooled rows (the inputs of mlps_out) and the per-voxel rows (the outputs of
    mlps_in) captured by hooks -> dict of everything the two paths must agree on"""
    from cpd_amd import ops
    pooled, fins, hooks = [], [], []
    for k in range(len(mod.nsamples)):
        hooks.append(mod.mlps_out[k].register_forward_pre_hook(lambda _m, args: pooled.append(args[0])))

        def keep(_m, _a, out):
            out.retain_grad()
            fins.append(out)
        hooks.append(mod.mlps_in[k].register_forward_hook(keep))
    sc = dict(scene)
    sc["features"] = scene["features"].clone().requires_grad_(True)
    if new_xyz_grad:
        sc["new_xyz"] = scene["new_xyz"].clone().requires_grad_(True)
    if not counts:
        sc["xyz_batch_cnt"] = None
    with ops.launch_log() as log:
        out = mod(**sc)
        loss = sum((p.reshape(p.shape[1], -1).t() * gk).sum() for p, gk in zip(pooled, grads)) + 0.0 * out.sum()
        loss.backward()
    for h in hooks:
        h.remove()
    res = dict(out=out.detach(), log=log.counts, dfeat=sc["features"].grad)
    for k in range(len(mod.nsamples)):
        bn = mod.mlps_pos[k][1]
        res["pooled%d" % k] = pooled[k].detach().reshape(pooled[k].shape[1], -1).t()
        res["dfin%d" % k] = fins[k].grad[0].t()
        res["dw%d" % k], res["dgamma%d" % k], res["dbeta%d" % k] = mod.mlps_pos[k][0].weight.grad[:, :, 0, 0], bn.weight.grad, bn.bias.grad
        res["rm%d" % k], res["rv%d" % k], res["nbt%d" % k] = bn.running_mean, bn.running_var, bn.num_batches_tracked
    return res


FUSED_KERNELS = {"voxel_pool_moments_kernel", "voxel_pool_max_train_kernel", "voxel_pool_max_train_grad_kernel"}
GROUP_KERNELS = {"group_points_kernel", "group_points_grad_kernel"}


def test_module_with_fused_train_matches_the_module_sequence(hip):
    from cpd_amd import roi_pool as rp
    scene = _scene()
    plain = _module([[8, 16, 16], [8, 32, 32]])
    fused = copy.deepcopy(plain)
    assert plain.fused_train is False and rp.set_fused_train(fused) == 1 and fused.fused_train is True
    assert list(plain.state_dict()) == list(fused.state_dict())
    g = torch.Generator().manual_seed(9)
    grads = [torch.randn(130, 16, generator=g).cuda(), torch.randn(130, 32, generator=g).cuda()]
    a = _run_module(plain, scene, grads)
    b = _run_module(fused, scene, grads, counts=False)                 # global rows: no per-sample row counts
    assert GROUP_KERNELS <= set(a["log"]) and not FUSED_KERNELS & set(a["log"]), a["log"]
    assert all(b["log"].get(k) == 2 for k in FUSED_KERNELS) and not GROUP_KERNELS & set(b["log"]), b["log"]
    empty = int((rp.voxel_query([1, 1, 1], 1.2, 8, scene["xyz"], scene["new_xyz"], scene["new_coords"][:, [0, 3, 2, 1]].contiguous(),
                                scene["voxel2point_indices"])[1]).sum())
    assert 0 < empty < 130                                             # the scene has empty and non-empty balls
    for k in (0, 1):
        err = float((a["pooled%d" % k] - b["pooled%d" % k]).abs().max())
        print("scale %d pooled: max |diff| %.3e" % (k, err))
        assert err <= 2e-5
        np.testing.assert_allclose(b["rm%d" % k].cpu().numpy(), a["rm%d" % k].cpu().numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(b["rv%d" % k].cpu().numpy(), a["rv%d" % k].cpu().numpy(), rtol=1e-5, atol=1e-6)
        assert int(a["nbt%d" % k]) == int(b["nbt%d" % k]) == 1
        for name in ("dfin", "dgamma", "dbeta"):
            _within(b["%s%d" % (name, k)], a["%s%d" % (name, k)].cpu(), 2e-5, "scale %d %s" % (k, name))
        np.testing.assert_allclose(b["dw%d" % k].cpu().numpy(), a["dw%d" % k].cpu().numpy(), rtol=1e-4, atol=1e-4)
    _within(b["dfeat"], a["dfeat"].cpu(), 2e-5, "d features")


def _fallback_cases():
    def bn_eval(mod):
        for seq in mod.mlps_pos:
            seq[1].eval()

    def attr(name, value):
        def f(mod):
            for seq in mod.mlps_pos:
                setattr(seq[1], name, value)
        return f
    return [("bn_eval", bn_eval, {}), ("no_running_stats", attr("track_running_stats", False), {}), ("no_affine", attr("affine", False), {}),
            ("no_momentum", attr("momentum", None), {}), ("width_24", None, {}), ("new_xyz_grad", None, dict(new_xyz_grad=True))]


@pytest.mark.parametrize("name,change,kw", _fallback_cases(), ids=[c[0] for c in _fallback_cases()])
def test_configurations_outside_the_fused_path_fall_back_bit_for_bit(hip, name, change, kw):
    from cpd_amd import roi_pool as rp
    scene = _scene()
    width = 24 if name == "width_24" else 16
    plain = _module([[8, width, width]])
    if change is not None:
        change(plain)
    fused = copy.deepcopy(plain)
    rp.set_fused_train(fused)
    assert not fused.fused_train_ready(scene["xyz"], scene["new_xyz"].clone().requires_grad_(bool(kw)))
    grads = [torch.randn(130, width, generator=torch.Generator().manual_seed(2)).cuda()]
    a, b = _run_module(plain, scene, grads, **kw), _run_module(fused, scene, grads, **kw)
    assert not FUSED_KERNELS & set(b["log"]) and "group_points_kernel" in b["log"], b["log"]
    for k in ("out", "pooled0", "rm0", "rv0", "nbt0"):
        assert torch.equal(a[k], b[k]), (name, k)


def test_a_single_slot_is_left_to_the_module_sequence(hip):
    mod = _module([[8, 16, 16]])
    mod.fused_train, mod.nsamples = True, [1]
    one = torch.zeros(1, 3).cuda()
    assert not mod._fused_scale(0, one, one) and mod._fused_scale(0, one, torch.zeros(2, 3).cuda())


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_proto_head_training_step_with_fused_pooling_matches_reference(golden, hip):
    """tests/test_gpu_roi_train.py's step (both pooling stacks of VoxelRCNNProtoHead) with the switch on, same constants. Every row
    holds at these constants, so no row is excluded for a near tie (a cell as in the module docstring feeding it) and the count printed is 0."""
    import types
    from test_gpu_roi_train import _cfg, _close
    from cpd_amd import ops, roi_pool as rp
    from cpd_amd.roi_head_train import VoxelRCNNProtoHead
    g = golden("proto_head")
    head = VoxelRCNNProtoHead(input_channels={"x_conv3": 8, "x_conv4": 12}, model_cfg=_cfg(), point_cloud_range=g["pcr"].tolist(),
                              voxel_size=[0.1, 0.1, 0.15], num_class=1)
    missing, unexpected = head.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("h.")}, strict=False)
    assert not unexpected and not missing
    head = head.cuda().train()
    assert rp.set_fused_train(head) == 4                               # two levels in each of the two stacks
    lv, lv_mm = {}, {}
    for name, shp in (("x_conv3", [11, 104, 104]), ("x_conv4", [5, 52, 52])):
        idx = torch.from_numpy(g[name + "_idx"]).cuda()
        for d, key in ((lv, "_feat"), (lv_mm, "_feat_mm")):
            f = torch.from_numpy(g[name + key]).cuda().requires_grad_(True)
            d[name] = types.SimpleNamespace(indices=idx, features=f, spatial_shape=shp, batch_size=2)
    bd = {"batch_size": 2, "batch_box_preds": torch.from_numpy(g["boxes"]).cuda(), "batch_cls_preds": torch.from_numpy(g["cls"]).cuda(),
          "gt_boxes": torch.from_numpy(g["gt"]).cuda(), "css_score": torch.from_numpy(g["css"]).cuda(), "multi_scale_3d_features": lv,
          "multi_scale_3d_features_mm": lv_mm, "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    with ops.launch_log() as log:
        head(bd)
    assert log.counts.get("voxel_pool_max_train_kernel") == 8 and "group_points_kernel" not in log.counts, log.counts
    assert all(int(m.num_batches_tracked) == 1 for m in head.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
    t0, t1 = head.forward_ret_dict["targets_dict0"], head.forward_ret_dict["targets_dict1"]
    np.testing.assert_allclose(t0["rois"].cpu().numpy(), g["t_rois"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(t0["roi_labels"].cpu().numpy(), g["t_roi_labels"])
    np.testing.assert_array_equal(t0["reg_valid_mask"].cpu().numpy(), g["t_reg_valid_mask"])
    for i, t in enumerate((t0, t1)):
        for k in ("shared_features", "rcnn_cls", "rcnn_reg"):
            _close(t[k].detach().cpu().numpy(), g["o%d_%s" % (i, k)], "branch %d %s" % (i, k))
    loss, tb = head.get_loss()
    assert abs(loss.item() - float(g["loss"])) <= 2e-4 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))
    with ops.launch_log() as log:
        loss.backward()
    assert log.counts.get("voxel_pool_max_train_grad_kernel") == 8 and "group_points_grad_kernel" not in log.counts, log.counts
    params = dict(head.named_parameters())
    n = 0
    for k in g.files:
        if k.startswith("g."):
            _close(params[k[2:]].grad.cpu().numpy(), g[k], "grad " + k[2:], rtol=1e-3, floor=1e-6)
            n += 1
    assert n >= 30
    for name in ("x_conv3", "x_conv4"):
        _close(lv[name].features.grad.cpu().numpy()[::4], g[name + "_grad4"], "d loss / d " + name, rtol=1e-3, floor=1e-7)
        _close(lv_mm[name].features.grad.cpu().numpy()[::4], g[name + "_grad4_mm"], "d loss / d mm " + name, rtol=1e-3, floor=1e-7)
    print("rows excluded for near ties: 0")


def test_voxel_rcnn_head_training_step_with_fused_pooling_matches_reference(golden, hip):
    """tests/test_gpu_rcnn_head_train.py's step (roi_pool.VoxelRCNNHead) with the switch on, same constants; no row excluded for a near tie"""
    from test_gpu_rcnn_head_train import _close, _fixture_batch, _fixture_head
    from cpd_amd import ops, roi_pool as rp
    g = golden("voxel_rcnn_head_train")
    head = _fixture_head(g).train()
    assert rp.set_fused_train(head) == 2
    bd = _fixture_batch(g)
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    with ops.launch_log() as log:
        head(bd)
    assert log.counts.get("voxel_pool_max_train_kernel") == 4 and "group_points_kernel" not in log.counts, log.counts
    t = head.forward_ret_dict
    np.testing.assert_allclose(t["rois"].cpu().numpy(), g["t_rois"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(t["roi_labels"].cpu().numpy(), g["t_roi_labels"])
    np.testing.assert_array_equal(t["reg_valid_mask"].cpu().numpy(), g["t_reg_valid_mask"])
    for k in ("rcnn_cls", "rcnn_reg"):
        _close(t[k].detach().cpu().numpy(), g["o_" + k], k)
    loss, tb = head.get_loss()
    want_loss = float(g["loss"])
    assert abs(loss.item() - want_loss) <= 2e-4 * abs(want_loss), (loss.item(), want_loss)
    with ops.launch_log() as log:
        loss.backward()
    assert log.counts.get("voxel_pool_max_train_grad_kernel") == 4 and "group_points_grad_kernel" not in log.counts, log.counts
    params = dict(head.named_parameters())
    n = 0
    for k in g.files:
        if k.startswith("g."):
            _close(params[k[2:]].grad.cpu().numpy(), g[k], "grad " + k[2:], rtol=1e-3, floor=1e-6)
            n += 1
    assert n >= 20
    for name in ("x_conv3", "x_conv4"):
        _close(bd["multi_scale_3d_features"][name].features.grad.cpu().numpy()[::4], g[name + "_grad4"], "d loss / d " + name,
               rtol=1e-3, floor=1e-7)
    print("rows excluded for near ties: 0")
