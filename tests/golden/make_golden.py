#!/usr/bin/env python3
"""Generate golden input/output vectors from the REFERENCE itself (run in the build container only).

What is executed here is the reference's own code, imported from /root/reference by file path:
  * cpd/models/backbones_3d/vfe/mean_vfe.py            -> MeanVFE.forward
  * cpd/models/backbones_2d/base_bev_backbone.py       -> BaseBEVBackbone.forward
  * cpd/models/dense_heads/center_head.py              -> SeparateHead.forward
  * cpd/models/model_utils/centernet_utils.py          -> _topk, decode_bbox_from_heatmap
  * cpd/models/model_utils/model_nms_utils.py          -> class_agnostic_nms
  * cpd/ops/iou3d_nms/src/iou3d_cpu.cpp (compiled: oracle/_ref/libiou3d_ref.so) -> boxes_iou_bev_cpu
The reference cannot be imported as a package here (spconv / numba / easydict / its CUDA
extensions are absent), so leaf files are loaded under a synthetic package `r` whose missing
siblings are empty modules. `numba` is replaced by an identity-decorator module: the only numba
user in these files (circle_nms, centernet_utils.py:80-104) is asserted unused by the reference
(l.161) and is never called here. `iou3d_nms_utils` (needs the CUDA extension) is replaced by a
module whose nms_gpu sorts by score exactly as iou3d_nms_utils.py:103-118 does and takes its IoUs
from the compiled reference iou3d_cpu.cpp, followed by the greedy scan of iou3d_nms.cpp:121-132.

Only DATA is written (tests/golden/*.npz): inputs, weights and the reference's outputs. No
reference source text is stored. Usage:  python tests/golden/make_golden.py
"""
import ctypes
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("CPD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
FP = ctypes.POINTER(ctypes.c_float)


class AttrDict(dict):
    """Minimal stand-in for easydict.EasyDict (attribute access + .get)."""
    __getattr__ = dict.__getitem__

    def __setattr__(self, k, v):
        self[k] = v


def _pkg(name):
    m = types.ModuleType(name)
    m.__path__ = []
    sys.modules[name] = m
    return m


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def ref_iou_lib():
    path = os.path.join(REPO, "oracle", "_ref", "libiou3d_ref.so")
    if not os.path.exists(path):
        raise SystemExit("build oracle/_ref first: make -C oracle ref")
    return ctypes.CDLL(path)


def ref_iou_bev(lib, a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    out = np.zeros((a.shape[0], b.shape[0]), np.float32)
    lib.ref_boxes_iou_bev_cpu(a.ctypes.data_as(FP), a.shape[0], b.ctypes.data_as(FP), b.shape[0],
                              out.ctypes.data_as(FP))
    return out


def greedy_keep(iou, thr):
    """Bitmask NMS on an IoU matrix of score-sorted boxes (iou3d_nms.cpp:117-133 semantics)."""
    n = iou.shape[0]
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= iou[i, i + 1:] > thr
    return np.asarray(keep, np.int64)


def setup_reference():
    for p in ["r", "r.models", "r.models.dense_heads", "r.models.model_utils", "r.models.backbones_3d",
              "r.models.backbones_3d.vfe", "r.models.backbones_2d", "r.utils", "r.ops", "r.ops.iou3d_nms"]:
        _pkg(p)
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (lambda f: f)
    sys.modules["numba"] = numba
    sys.modules["r.utils.box_utils"] = types.ModuleType("r.utils.box_utils")
    lib = ref_iou_lib()

    nms_mod = types.ModuleType("r.ops.iou3d_nms.iou3d_nms_utils")

    def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
        order = scores.sort(0, descending=True)[1]
        if pre_maxsize is not None:
            order = order[:pre_maxsize]
        b = boxes[order].contiguous().numpy()
        keep = greedy_keep(ref_iou_bev(lib, b, b), thresh)
        return order[torch.from_numpy(keep)].contiguous(), None

    nms_mod.nms_gpu = nms_gpu
    sys.modules["r.ops.iou3d_nms.iou3d_nms_utils"] = nms_mod
    sys.modules["r.ops.iou3d_nms"].iou3d_nms_utils = nms_mod

    m = {}
    m["vfe_template"] = _load("r.models.backbones_3d.vfe.vfe_template", "cpd/models/backbones_3d/vfe/vfe_template.py")
    m["mean_vfe"] = _load("r.models.backbones_3d.vfe.mean_vfe", "cpd/models/backbones_3d/vfe/mean_vfe.py")
    m["bev"] = _load("r.models.backbones_2d.base_bev_backbone", "cpd/models/backbones_2d/base_bev_backbone.py")
    m["loss_utils"] = _load("r.utils.loss_utils", "cpd/utils/loss_utils.py")
    m["centernet_utils"] = _load("r.models.model_utils.centernet_utils", "cpd/models/model_utils/centernet_utils.py")
    m["model_nms_utils"] = _load("r.models.model_utils.model_nms_utils", "cpd/models/model_utils/model_nms_utils.py")
    sys.modules["r.models.model_utils"].centernet_utils = m["centernet_utils"]
    sys.modules["r.models.model_utils"].model_nms_utils = m["model_nms_utils"]
    sys.modules["r.utils"].loss_utils = m["loss_utils"]
    m["center_head"] = _load("r.models.dense_heads.center_head", "cpd/models/dense_heads/center_head.py")
    m["lib"] = lib
    return m


def rand_boxes(rng, n, span=30.0):
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-span, span, (n, 2))
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3:6] = np.exp(rng.normal(0, 0.25, (n, 3))) * np.array([4.7, 2.1, 1.7])
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def adversarial_boxes(rng):
    """identical / nested / touching / theta ~ +-pi / tiny / near-duplicate boxes."""
    base = rand_boxes(rng, 24, span=6.0)
    out = [base]
    out.append(base[:6].copy())                                   # identical
    nested = base[:6].copy(); nested[:, 3:5] *= 0.5; out.append(nested)
    touch = base[:6].copy(); touch[:, 6] = 0; t2 = touch.copy(); t2[:, 0] += t2[:, 3]; out += [touch, t2]
    pi = base[:6].copy(); pi[:, 6] = np.float32(np.pi) - 1e-4; p2 = pi.copy(); p2[:, 6] = -np.float32(np.pi) + 1e-4
    out += [pi, p2]
    tiny = base[:6].copy(); tiny[:, 3:5] = 1e-3; out.append(tiny)
    dup = base[:12].copy(); dup[:, :2] += rng.normal(0, 0.05, (12, 2)); dup[:, 6] += rng.normal(0, 0.02, 12)
    out.append(dup)
    ax = base[:6].copy(); ax[:, 6] = np.float32(np.pi / 2); out.append(ax)
    return np.concatenate(out, 0).astype(np.float32)


def borderline_free(iou, thr, margin=2e-4):
    return not np.any(np.abs(iou - thr) < margin)


def nms_large(m):
    """NMS_PRE_MAXSIZE-sized set (4096 boxes, 64 mask words per row: the multi-block scan of the device kernel) through the
    reference's class_agnostic_nms. Own RNG: adding this section moves no other fixture."""
    rng = np.random.default_rng(4096)
    lib = m["lib"]
    n, thr, span = 4096, 0.7, 96.0
    for attempt in range(400):
        bx = rand_boxes(rng, n, span=span)
        k = n // 10
        bx[n - k:] = bx[:k]
        bx[n - k:, :2] += rng.normal(0, 0.25, (k, 2)).astype(np.float32)
        bx[n - k:, 6] += rng.normal(0, 0.05, k).astype(np.float32)
        sc = rng.permutation(n).astype(np.float32) / n + 0.001
        order = np.argsort(-sc, kind="stable")
        iou = ref_iou_bev(lib, bx[order], bx[order])
        if borderline_free(iou[np.triu_indices(n, 1)], thr):
            break
    else:
        raise RuntimeError("no borderline-free 4096-box set")
    cfgn = AttrDict(NMS_TYPE="nms_gpu", NMS_THRESH=thr, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=4096)
    sel, sel_sc = m["model_nms_utils"].class_agnostic_nms(
        box_scores=torch.from_numpy(sc), box_preds=torch.from_numpy(bx), nms_config=cfgn, score_thresh=None)
    np.savez_compressed(os.path.join(HERE, "nms_n4096.npz"), boxes=bx, scores=sc, thr=np.float32(thr), selected=sel.numpy(),
                        selected_scores=sel_sc.numpy())
    print("nms_n4096: %d boxes -> %d kept (attempt %d)" % (n, sel.shape[0], attempt))


def atss(m):
    """ATSSTargetAssigner.assign_targets (atss_target_assigner.py:16-141) run as the reference wrote it, on the reference's own
    AnchorGenerator / ResidualCoder / common_utils.rotate_points_along_z; its CUDA-only boxes_iou_bev is served by the
    reference's CPU implementation (iou3d_cpu.cpp compiled in oracle/_ref). Two cases: topk = 8 on the usual anchors (two
    rotations per location: the pair is equidistant from every box, an even k never cuts through a pair) and topk = 9 on
    one-rotation anchors (no ties) -- an odd k on two-rotation anchors cuts a tied pair, torch.topk leaves that order
    unspecified, and the choice moves the mean + std threshold (seen: 1 label of 16,224 differs from the lower-index rule).
    Own RNG: adding this section moves no other fixture."""
    lib = m["lib"]
    torch.Tensor.cuda = lambda self, *a, **k: self
    for pkg in ["r.models.dense_heads.target_assigner"]:
        if pkg not in sys.modules:
            _pkg(pkg)
    cu = _load("r.utils.common_utils", "cpd/utils/common_utils.py")
    sys.modules["r.utils"].common_utils = cu
    bc = _load("r.utils.box_coder_utils", "cpd/utils/box_coder_utils.py")
    ag = _load("r.models.dense_heads.target_assigner.anchor_generator",
               "cpd/models/dense_heads/target_assigner/anchor_generator.py")
    nms_mod = sys.modules["r.ops.iou3d_nms.iou3d_nms_utils"]
    nms_mod.boxes_iou_bev = lambda a, b: torch.from_numpy(ref_iou_bev(lib, a.contiguous().numpy(), b.contiguous().numpy()))
    at = _load("r.models.dense_heads.target_assigner.atss_target_assigner",
               "cpd/models/dense_heads/target_assigner/atss_target_assigner.py")
    g = np.random.default_rng(1912)
    pcr = np.array([-20.8, -20.8, -2.0, 20.8, 20.8, 4.0], np.float32)
    agc = [AttrDict(class_name="Vehicle", anchor_sizes=[[4.7, 2.1, 1.7]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0],
                    align_center=False, feature_map_stride=8),
           AttrDict(class_name="Pedestrian", anchor_sizes=[[0.91, 0.86, 1.73]], anchor_rotations=[0, 1.57],
                    anchor_bottom_heights=[0], align_center=False, feature_map_stride=8),
           AttrDict(class_name="Cyclist", anchor_sizes=[[1.78, 0.84, 1.78]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0],
                    align_center=False, feature_map_stride=8)]
    H = W = 52
    anchors_list, _ = ag.AnchorGenerator(anchor_range=pcr, anchor_generator_config=agc).generate_anchors([[W, H]] * 3)
    n_gt = 11
    sizes = np.array([[4.7, 2.1, 1.7], [0.91, 0.86, 1.73], [1.78, 0.84, 1.78]])
    gt = np.zeros((2, n_gt + 3, 8), np.float32)
    for b in range(2):
        cls = g.integers(1, 4, n_gt)
        for i in range(n_gt - b * 2):                                 # the second frame has two more padding rows
            gt[b, i] = [g.uniform(-19, 19), g.uniform(-19, 19), g.uniform(-0.5, 0.5), *(sizes[cls[i] - 1] * g.uniform(0.85, 1.15, 3)),
                        g.uniform(-3.1, 3.1), cls[i]]
    gt[0, 3, :2] = gt[0, 2, :2] + 0.3                                 # two boxes that compete for the same anchors
    gt[0, 3, 3:6] = gt[0, 2, 3:6]
    agc1 = [AttrDict(dict(c, anchor_rotations=[0.6 + 0.3 * i])) for i, c in enumerate(agc)]        # one rotation: no tied pairs
    anchors_1rot, _ = ag.AnchorGenerator(anchor_range=pcr, anchor_generator_config=agc1).generate_anchors([[W, H]] * 3)
    out = {"pcr": pcr, "hw": np.array([H, W]), "gt": gt, "anchors_k8": torch.stack(anchors_list).numpy(),
           "anchors_k9": torch.stack(anchors_1rot).numpy()}
    coder = bc.ResidualCoder()
    for k, alist in ((8, anchors_list), (9, anchors_1rot)):
        asg = at.ATSSTargetAssigner(topk=k, box_coder=coder, match_height=False)
        t = asg.assign_targets([a.clone() for a in alist], torch.from_numpy(gt.copy()))
        t1 = asg.assign_targets(alist[0].clone(), torch.from_numpy(gt.copy()))
        out["labels_k%d" % k] = t["box_cls_labels"].numpy()
        out["reg_targets_k%d" % k] = t["box_reg_targets"].numpy()
        out["reg_weights_k%d" % k] = t["reg_weights"].numpy()
        out["labels_single_k%d" % k] = t1["box_cls_labels"].numpy()
        print("atss k=%d: %d positive anchors of %d" % (k, int((t["box_cls_labels"] > 0).sum()), t["box_cls_labels"].numel()))
    np.savez_compressed(os.path.join(HERE, "atss.npz"), **out)


def _load_roi_stack(m):
    """The reference's second-stage Python stack on CPU: voxel_pool_modules / voxel_query_utils / pointnet2_utils,
    proposal_target_layer, roi_head_template, voxel_rcnn_head, bbloss, loss_utils + box_utils, common_utils -- all loaded by
    file path. The CUDA extensions they call are served by the oracle (voxel query, grouping and its scatter-add backward, 3-D
    IoU) and by the reference's compiled CPU IoU (proposal NMS). Module loading only: no random numbers are drawn here."""
    import types as _t
    sys.path.insert(0, REPO)
    from oracle.binding import Oracle
    orc = Oracle()
    torch.Tensor.cuda = lambda self, *a, **k: self
    for pkg in ["r.ops.pointnet2", "r.ops.pointnet2.pointnet2_stack", "r.models.roi_heads", "r.models.roi_heads.target_assigner"]:
        if pkg not in sys.modules:
            _pkg(pkg)
    ext = _t.ModuleType("r.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda")

    def voxel_query_wrapper(M, Z, Y, X, nsample, radius, zr, yr, xr, new_xyz, xyz, new_coords, point_indices, idx):
        idx.copy_(torch.from_numpy(orc.voxel_query([zr, yr, xr], radius, nsample, xyz.numpy(), new_xyz.numpy(), new_coords.numpy(),
                                                   point_indices.numpy())))

    def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, output):
        output.copy_(torch.from_numpy(orc.group_points(features.detach().numpy(), features_batch_cnt.numpy(), idx.numpy(),
                                                       idx_batch_cnt.numpy())))

    def group_points_grad_wrapper(B, M, C, N, nsample, grad_out, idx, idx_batch_cnt, features_batch_cnt, grad_features):
        # group_points_grad_kernel_stack (group_points_gpu.cu:9-36): scatter-add of the grouped gradient, in float64 here
        go, ix = grad_out.numpy().astype(np.float64), idx.numpy()
        starts_f = np.concatenate([[0], np.cumsum(features_batch_cnt.numpy())[:-1]])
        pt_batch = np.repeat(np.arange(B), idx_batch_cnt.numpy())
        rows = starts_f[pt_batch][:, None] + ix                                        # (M, nsample)
        acc = np.zeros((N, C))
        np.add.at(acc, rows.reshape(-1), go.transpose(0, 2, 1).reshape(-1, C))
        grad_features.copy_(torch.from_numpy(acc.astype(np.float32)))

    ext.voxel_query_wrapper, ext.group_points_wrapper, ext.group_points_grad_wrapper = voxel_query_wrapper, group_points_wrapper, group_points_grad_wrapper
    sys.modules[ext.__name__] = ext
    sys.modules["r.ops.pointnet2.pointnet2_stack"].pointnet2_stack_cuda = ext
    torch.cuda.IntTensor = lambda *sz: torch.zeros(*sz, dtype=torch.int32)
    torch.cuda.FloatTensor = lambda *sz: torch.zeros(*sz, dtype=torch.float32)
    stack = sys.modules["r.ops.pointnet2.pointnet2_stack"]
    stack.pointnet2_utils = _load("r.ops.pointnet2.pointnet2_stack.pointnet2_utils", "cpd/ops/pointnet2/pointnet2_stack/pointnet2_utils.py")
    stack.voxel_query_utils = _load("r.ops.pointnet2.pointnet2_stack.voxel_query_utils", "cpd/ops/pointnet2/pointnet2_stack/voxel_query_utils.py")
    vp = _load("r.ops.pointnet2.pointnet2_stack.voxel_pool_modules", "cpd/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py")
    stack.voxel_pool_modules = vp
    sys.modules["r.ops.pointnet2"].pointnet2_stack = stack
    cu = _load("r.utils.common_utils", "cpd/utils/common_utils.py")
    sys.modules["r.utils"].common_utils = cu
    for stub in ["r.ops.roiaware_pool3d", "r.ops.roiaware_pool3d.roiaware_pool3d_utils"]:
        sys.modules.setdefault(stub, _t.ModuleType(stub))
    sys.modules["r.ops"].roiaware_pool3d = sys.modules["r.ops.roiaware_pool3d"]
    sys.modules["r.ops.roiaware_pool3d"].roiaware_pool3d_utils = sys.modules["r.ops.roiaware_pool3d.roiaware_pool3d_utils"]
    sys.modules["scipy.spatial"] = __import__("scipy.spatial").spatial
    bu = _load("r.utils.box_utils", "cpd/utils/box_utils.py")
    sys.modules["r.utils"].box_utils = bu
    m["loss_utils"].box_utils = bu                                     # setup_reference() loaded loss_utils against an empty stub
    sys.modules["r.utils"].box_coder_utils = _load("r.utils.box_coder_utils", "cpd/utils/box_coder_utils.py")
    spu = _t.ModuleType("r.utils.spconv_utils")                        # generate_voxel2pinds only (the file imports spconv at top)
    spu.generate_voxel2pinds = lambda t: torch.from_numpy(orc.voxel2pinds(t.indices.numpy().astype(np.int32), t.batch_size, list(t.spatial_shape)))
    sys.modules["r.utils.spconv_utils"] = spu
    sys.modules["r.utils"].spconv_utils = spu
    nms_mod = sys.modules["r.ops.iou3d_nms.iou3d_nms_utils"]
    nms_mod.boxes_iou3d_gpu = lambda a, b: torch.from_numpy(orc.boxes_iou3d(a.contiguous().numpy(), b.contiguous().numpy()))
    _load("r.utils.bbloss", "cpd/utils/bbloss.py")
    _load("r.utils.odiou_loss", "cpd/utils/odiou_loss.py")
    ptl = _load("r.models.roi_heads.target_assigner.proposal_target_layer", "cpd/models/roi_heads/target_assigner/proposal_target_layer.py")
    rht = _load("r.models.roi_heads.roi_head_template", "cpd/models/roi_heads/roi_head_template.py")
    vrh = _load("r.models.roi_heads.voxel_rcnn_head", "cpd/models/roi_heads/voxel_rcnn_head.py")
    return dict(orc=orc, vp=vp, ptl=ptl, rht=rht, vrh=vrh, cu=cu)


def proto_head(m):
    """VoxelRCNNProtoHead in TRAINING mode (voxel_rcnn_head.py:16-662): proposal layer (class-agnostic NMS), proposal target
    sampling (np.random / torch.randint under recorded seeds), canonical targets, both pooling branches with batch-statistics
    BatchNorm, get_loss and its autograd gradients, all from the reference's own classes on CPU (_load_roi_stack). DP_RATIO = 0:
    dropout masks are not reproducible across devices. Own RNG: adding this section moves no other fixture."""
    R = _load_roi_stack(m)
    pool = lambda: AttrDict(FEATURES_SOURCE=["x_conv3", "x_conv4"], PRE_MLP=True, GRID_SIZE=2, POOL_LAYERS=AttrDict(
        x_conv3=AttrDict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[0.6, 1.2], NSAMPLE=[8, 8], POOL_METHOD="max_pool"),
        x_conv4=AttrDict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[1.2, 2.4], NSAMPLE=[8, 8], POOL_METHOD="max_pool")))
    cfg = AttrDict(
        CLASS_AGNOSTIC=True, ROI_GRID_POOL=pool(), ROI_GRID_POOL_PROTO=pool(), SHARED_FC=[48, 48], CLS_FC=[32, 32], REG_FC=[32, 32], DP_RATIO=0.0,
        TARGET_CONFIG=AttrDict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=24, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou",
                               CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.02, CLS_BG_THRESH_LO=0.01, HARD_BG_RATIO=0.1, REG_FG_THRESH=0.3),
        LOSS_CONFIG=AttrDict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True, GRID_3D_IOU_LOSS=False,
                             LOSS_WEIGHTS=AttrDict(rcnn_proto_weight=1.0, rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0,
                                                   rcnn_iou3d_weight=1.0, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8])),
        NMS_CONFIG=AttrDict(TRAIN=AttrDict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=400, NMS_POST_MAXSIZE=60, NMS_THRESH=0.8)))
    pcr = np.array([-20.8, -20.8, -2.0, 20.8, 20.8, 4.0], np.float32)
    g = np.random.default_rng(1662)
    torch.manual_seed(1662)
    head = R["vrh"].VoxelRCNNProtoHead(input_channels={"x_conv3": 8, "x_conv4": 12}, model_cfg=cfg, point_cloud_range=pcr,
                                       voxel_size=[0.1, 0.1, 0.15], num_class=1).train()
    with torch.no_grad():
        for mm in head.modules():
            if isinstance(mm, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mm.weight.uniform_(0.6, 1.4); mm.bias.normal_(0, 0.2)
        for stack in (head.cls_layers, head.reg_layers, head.cls_layers_P, head.reg_layers_P):
            stack[-1].weight.normal_(0, 0.08)
    from types import SimpleNamespace
    B, n_gt = 2, 7
    gt = np.zeros((B, n_gt + 2, 8), np.float32)
    sizes = np.array([[4.6, 2.0, 1.7], [0.9, 0.8, 1.7], [1.8, 0.8, 1.7]])
    for b in range(B):
        for i in range(n_gt - b):
            c = g.integers(1, 4)
            gt[b, i] = [g.uniform(-17, 17), g.uniform(-17, 17), g.uniform(-0.3, 0.6), *(sizes[c - 1] * g.uniform(0.9, 1.1, 3)), g.uniform(-3.1, 3.1), c]
    css = np.zeros((B, n_gt + 2), np.float32)
    css[:, :n_gt] = g.uniform(0.2, 1.0, (B, n_gt))
    css[0, 1] = 0.0                                                    # a box whose prototype confidence switches its RoIs off
    # dense-head output the proposal layer sees: jittered copies of the boxes (several IoU levels) + clutter
    n_prop = 420
    boxes = np.zeros((B, n_prop, 7), np.float32)
    cls = g.normal(-2.0, 1.0, (B, n_prop, 3)).astype(np.float32)
    for b in range(B):
        ng = n_gt - b
        for j in range(n_prop):
            if j < 300:
                src = gt[b, j % ng, :7].copy()
                lvl = [0.03, 0.12, 0.35][(j // ng) % 3]
                src[:3] += g.normal(0, lvl, 3) * [1.0, 1.0, 0.3]
                src[3:6] *= g.uniform(1 - lvl, 1 + lvl, 3)
                src[6] += g.normal(0, lvl)
                boxes[b, j] = src
                cls[b, j, int(gt[b, j % ng, 7]) - 1] = g.normal(1.5, 1.0)
            else:
                boxes[b, j] = [g.uniform(-18, 18), g.uniform(-18, 18), g.uniform(-0.3, 0.6), *g.uniform(0.7, 4.5, 3), g.uniform(-3.1, 3.1)]
    lv, lv_mm = {}, {}
    for name, shp, ch, nvox in (("x_conv3", [11, 104, 104], 8, 1800), ("x_conv4", [5, 52, 52], 12, 700)):
        st = 4 if name == "x_conv3" else 8
        cells = [np.stack([g.integers(0, B, nvox), g.integers(0, shp[0], nvox), g.integers(0, shp[1], nvox), g.integers(0, shp[2], nvox)], 1)]
        for b in range(B):                                             # dense clusters of voxels inside every box: no empty balls there
            for i in range(n_gt - b):
                ctr = ((gt[b, i, :3] - pcr[:3]) / (np.array([0.1, 0.1, 0.15]) * st))
                pts = ctr[None] + g.uniform(-1, 1, (40, 3)) * (gt[b, i, 3:6] / (np.array([0.1, 0.1, 0.15]) * st)) * 0.6
                cz = np.clip(np.floor(pts[:, [2, 1, 0]]).astype(int), 0, np.array(shp) - 1)
                cells.append(np.concatenate([np.full((40, 1), b), cz], 1))
        cl = np.unique(np.concatenate(cells), axis=0).astype(np.int32)
        for d, seed in ((lv, 1), (lv_mm, 2)):
            f = torch.randn(cl.shape[0], ch, generator=torch.Generator().manual_seed(1662 + seed + ch)).requires_grad_(True)
            d[name] = SimpleNamespace(indices=torch.from_numpy(cl), features=f, spatial_shape=shp, batch_size=B)
    bd = {"batch_size": B, "batch_box_preds": torch.from_numpy(boxes), "batch_cls_preds": torch.from_numpy(cls), "gt_boxes": torch.from_numpy(gt),
          "css_score": torch.from_numpy(css), "multi_scale_3d_features": lv, "multi_scale_3d_features_mm": lv_mm,
          "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}
    sd0 = {"h." + k: v.detach().clone().numpy() for k, v in head.state_dict().items()}
    np.random.seed(77)
    torch.manual_seed(77)
    head(bd)
    loss, tb = head.get_loss()
    loss.backward()
    t0, t1 = head.forward_ret_dict["targets_dict0"], head.forward_ret_dict["targets_dict1"]
    out = dict(sd0)
    out.update(pcr=pcr, gt=gt, css=css, boxes=boxes, cls=cls, seed=np.int64(77), loss=np.float64(loss.item()), rcnn_loss=np.float64(tb["rcnn_loss"]))
    for name in ("x_conv3", "x_conv4"):
        out[name + "_idx"] = lv[name].indices.numpy()
        out[name + "_feat"], out[name + "_feat_mm"] = lv[name].features.detach().numpy(), lv_mm[name].features.detach().numpy()
        out[name + "_grad4"], out[name + "_grad4_mm"] = lv[name].features.grad.numpy()[::4], lv_mm[name].features.grad.numpy()[::4]   # every 4th row
    for k in ("rois", "gt_of_rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask", "rcnn_cls_labels"):
        out["t_" + k] = t0[k].detach().numpy()
    out["t_css"] = t0["additional_data"]["css_score"].numpy()
    for i, t in enumerate((t0, t1)):
        for k in ("rcnn_cls", "rcnn_reg", "shared_features"):
            out["o%d_%s" % (i, k)] = t[k].detach().numpy()
    for k, prm in head.named_parameters():
        if prm.grad is not None and (k.endswith("3.weight") or "mlps_pos" in k or k.startswith("shared_fc_layers.0") or k.endswith("0.0.weight")):
            out["g." + k] = prm.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "proto_head.npz"), **out)
    print("proto_head: loss %.6f, %d fg of %d rois, %d gradient arrays" % (loss.item(), int(t0["reg_valid_mask"].sum()),
                                                                           t0["reg_valid_mask"].numel(), sum(k.startswith("g.") for k in out)))


def target_layer_x(m):
    """ProposalTargetLayer.forward (proposal_target_layer.py:32-196, 198-362) with the PER-CLASS threshold lists of CLS_SCORE_TYPE
    `roi_iou_x` and `roi_ioud_x` (l.57-80, 128-184, 258-259, 297-322), with and without ENABLE_HARD_SAMPLING, from the reference's own
    class on CPU (_load_roi_stack: its boxes_iou3d_gpu is the oracle's) under recorded seeds. Own RNG: moves no other fixture."""
    R = _load_roi_stack(m)
    g = np.random.default_rng(2580)
    B, n_gt, n_roi = 2, 9, 300
    sizes = np.array([[4.6, 2.0, 1.7], [0.9, 0.8, 1.7], [1.8, 0.8, 1.7]])
    gt = np.zeros((B, n_gt + 2, 8), np.float32)
    for b in range(B):
        for i in range(n_gt - b):
            c = 1 + (i % 3)
            gt[b, i] = [g.uniform(-17, 17), g.uniform(-17, 17), g.uniform(-0.3, 0.6), *(sizes[c - 1] * g.uniform(0.9, 1.1, 3)), g.uniform(-3.1, 3.1), c]
    rois = np.zeros((B, n_roi, 7), np.float32)
    labels = np.zeros((B, n_roi), np.int64)
    for b in range(B):
        ng = n_gt - b
        for j in range(n_roi):
            if j < 240:
                src = gt[b, j % ng, :7].copy()
                lvl = [0.02, 0.08, 0.2, 0.4][(j // ng) % 4]
                src[:3] += g.normal(0, lvl, 3) * [1.0, 1.0, 0.3]
                src[3:6] *= g.uniform(1 - lvl, 1 + lvl, 3)
                src[6] += g.normal(0, 2 * lvl)
                rois[b, j] = src
                labels[b, j] = int(gt[b, j % ng, 7])
            else:
                rois[b, j] = [g.uniform(-18, 18), g.uniform(-18, 18), g.uniform(-0.3, 0.6), *g.uniform(0.7, 4.5, 3), g.uniform(-3.1, 3.1)]
                labels[b, j] = g.integers(1, 4)
    scores = g.uniform(0, 1, (B, n_roi)).astype(np.float32)
    out = dict(gt=gt, rois=rois, roi_labels=labels, roi_scores=scores)
    case = 0
    for kind in ("roi_iou_x", "roi_ioud_x"):
        for hard in (False, True):
            cfg = AttrDict(ROI_PER_IMAGE=64, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE=kind,
                           CLS_FG_THRESH=[0.75, 0.6, 0.65], CLS_BG_THRESH=[0.25, 0.15, 0.2], CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8,
                           REG_FG_THRESH=[0.55, 0.4, 0.45], DIRECTION_MIN=0.1, DIRECTION_MAX=0.9, ENABLE_HARD_SAMPLING=hard,
                           HARD_SAMPLING_THRESH=[0.3, 0.2, 0.25], HARD_SAMPLING_RATIO=[0.5, 0.25, 0.34])
            layer = R["ptl"].ProposalTargetLayer(roi_sampler_cfg=cfg)
            seed = 300 + case
            np.random.seed(seed)
            torch.manual_seed(seed)
            t = layer.forward({"batch_size": B, "rois": torch.from_numpy(rois), "roi_scores": torch.from_numpy(scores),
                               "roi_labels": torch.from_numpy(labels), "gt_boxes": torch.from_numpy(gt)})
            pre = "c%d_" % case
            out[pre + "kind"] = np.int64(0 if kind == "roi_iou_x" else 1)
            out[pre + "hard"], out[pre + "seed"] = np.int64(hard), np.int64(seed)
            for k in ("rois", "gt_of_rois", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask", "rcnn_cls_labels"):
                out[pre + k] = t[k].numpy()
            print("target_layer_x case %d (%s, hard %d): %d reg-valid of %d, cls labels in [%.3f, %.3f]" %
                  (case, kind, hard, int(t["reg_valid_mask"].sum()), t["reg_valid_mask"].numel(), float(t["rcnn_cls_labels"].min()),
                   float(t["rcnn_cls_labels"].max())))
            case += 1
    out["n_cases"] = np.int64(case)
    np.savez_compressed(os.path.join(HERE, "target_layer_x.npz"), **out)


PROTO_NAMES = ["Vehicle", "Pedestrian", "Cyclist", "Dis_Small", "Sign"]


def proto_crop(m):
    """sample_prototype_cpu (waymo_unsupervised_dataset.py:205-331) executed from the reference file itself (the method's source
    is cut out of the file at generation time -- the dataset module's import chain is not needed for it -- and run with numpy,
    a temporary prototype pickle and the reference's compiled points_in_boxes_cpu from oracle/_ref). Two scenes: coin 0 and 1.
    Class names are stored as indices into PROTO_NAMES. Own RNG: adding this section moves no other fixture."""
    import ast
    import pickle
    import tempfile
    sys.path.insert(0, REPO)
    from oracle.binding import load_reference_points_in_boxes
    ref_pib = load_reference_points_in_boxes()
    if ref_pib is None:
        raise SystemExit("build oracle/_ref first: make -C oracle ref")
    path = os.path.join(REF, "cpd/datasets/waymo_unsupervised/waymo_unsupervised_dataset.py")
    src = open(path).read()
    fn = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "sample_prototype_cpu"][0]
    import textwrap
    ns = {"np": np, "os": os, "pickle": pickle,
          "roiaware_pool3d_utils": types.SimpleNamespace(points_in_boxes_cpu=lambda pts, boxes: ref_pib(np.asarray(boxes)[:, :7], np.asarray(pts)[:, :3]))}
    exec(textwrap.dedent(ast.get_source_segment(src, fn)), ns)
    sample = ns["sample_prototype_cpu"]
    rng = np.random.default_rng(205)
    sizes = {"Vehicle": [4.7, 2.1, 1.7], "Pedestrian": [0.9, 0.85, 1.7], "Cyclist": [1.8, 0.85, 1.75], "Dis_Small": [0.5, 0.5, 0.6],
             "Sign": [0.3, 0.3, 2.0]}
    proto_set = {"proto_points_set": {}}
    for name in ("Vehicle", "Pedestrian", "Cyclist"):
        proto_set["proto_points_set"][name] = {}
        for pid in range(3):
            box = np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-0.5, 0.5), *(np.array(sizes[name]) * rng.uniform(0.9, 1.1, 3)),
                            rng.uniform(-3.1, 3.1)])
            loc = rng.uniform(-0.62, 0.62, (150, 3)) * box[3:6]           # some points fall outside the box and are cropped
            c, s_ = np.cos(box[6]), np.sin(box[6])
            pts = np.stack([loc[:, 0] * c - loc[:, 1] * s_ + box[0], loc[:, 0] * s_ + loc[:, 1] * c + box[1], loc[:, 2] + box[2],
                            rng.uniform(0, 1, 150)], 1).astype(np.float32)
            proto_set["proto_points_set"][name][pid] = {"points": pts, "box": box}
    cfg = AttrDict(InitLabelGenerator="gen", RefinerConfig=AttrDict(
        DiscardThreshMax={"Vehicle": 0.8, "Pedestrian": 0.7, "Cyclist": 0.7}, DiscardThreshMin={"Vehicle": 0.3, "Pedestrian": 0.2, "Cyclist": 0.25}))
    out = {}
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "seq"))
        with open(os.path.join(root, "seq", "seq_outline_gen_CSS_proto.pkl"), "wb") as f:
            pickle.dump(proto_set, f)
        for scene in range(2):
            k = 14
            names = [PROTO_NAMES[i] for i in rng.integers(0, 5, k)]
            names[0], names[1], names[2] = "Vehicle", "Pedestrian", "Cyclist"
            boxes = np.zeros((k, 7))
            for i, nme in enumerate(names):
                boxes[i] = [rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(-0.5, 0.5), *(np.array(sizes[nme]) * rng.uniform(0.9, 1.1, 3)),
                            rng.uniform(-3.1, 3.1)]
            boxes[3, :2] = [70.0, 40.0]                                 # beyond 75 m: dropped, and its points are discarded
            score = rng.uniform(0.05, 0.95, k)
            score[0], score[1] = 0.9, 0.1                               # clamped above / rejected below the thresholds
            pid = rng.integers(-1, 3, k)
            pid[0], pid[2] = 1, 2
            bg = np.concatenate([rng.uniform(-75, 75, (2500, 2)), rng.uniform(-2, 3, (2500, 1)), rng.uniform(0, 1, (2500, 2))], 1)
            obj = []
            for b in boxes:                                             # clusters in and around every box
                loc = rng.uniform(-0.7, 0.7, (60, 3)) * b[3:6]
                c, s_ = np.cos(b[6]), np.sin(b[6])
                obj.append(np.stack([loc[:, 0] * c - loc[:, 1] * s_ + b[0], loc[:, 0] * s_ + loc[:, 1] * c + b[1], loc[:, 2] + b[2],
                                     rng.uniform(0, 1, 60), rng.uniform(0, 1, 60)], 1))
            points = np.concatenate([bg] + obj).astype(np.float32)
            points = points[rng.permutation(len(points))]
            for seed in range(1000):                                    # a seed whose coin is `scene`
                np.random.seed(seed)
                if np.random.randint(2) == scene:
                    break
            np.random.seed(seed)
            good, proto, nb, nc, nsc, nid = sample(None, "seq", root, points, boxes, names, score, pid, cfg)
            np.random.seed(seed)
            coin = np.random.randint(2)
            crop = ref_pib(boxes, points[:, :3])
            disc = np.ones(k, bool)
            disc[[i for i in range(k) if any((boxes[i] == b).all() for b in nb)]] = False
            n_good_full = int((crop[disc].sum(0) == 0).sum()) if disc.any() else len(points)
            perm = np.random.permutation(n_good_full) if coin else np.zeros(0, np.int64)
            pre = "s%d_" % scene
            out.update({pre + "points": points, pre + "boxes": boxes, pre + "names": np.array([PROTO_NAMES.index(n) for n in names]),
                        pre + "score": score, pre + "proto_id": pid, pre + "coin": np.int64(coin), pre + "perm": perm,
                        pre + "good": good, pre + "proto": proto.astype(np.float32), pre + "new_boxes": nb,   # proto: float64 in the reference, stored rounded
                        pre + "new_names": np.array([PROTO_NAMES.index(n) for n in nc]), pre + "new_score": nsc, pre + "new_id": nid})
            print("proto_crop scene %d: coin %d, %d points -> good %d, proto %d (%d boxes kept of %d)" % (scene, coin, len(points), len(good),
                                                                                                   len(proto), len(nb), k))
    for name in ("Vehicle", "Pedestrian", "Cyclist"):
        for pid_ in range(3):
            e = proto_set["proto_points_set"][name][pid_]
            out["set_%s_%d_points" % (name, pid_)] = e["points"]
            out["set_%s_%d_box" % (name, pid_)] = e["box"]
    out["thr_max"] = np.array([0.8, 0.7, 0.7])
    out["thr_min"] = np.array([0.3, 0.2, 0.25])
    np.savez_compressed(os.path.join(HERE, "proto_crop.npz"), **out)


def points_in_boxes_fixture(m):
    """points_in_boxes_cpu (cpd/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:143-168, compiled from where it lies: oracle/_ref)
    on boxes x points with points placed on / next to every face and on the MARGIN = 1e-2 shell. The GPU box reads this
    file; the compiled reference stays in the build container. Own RNG."""
    sys.path.insert(0, REPO)
    from oracle.binding import load_reference_points_in_boxes
    ref = load_reference_points_in_boxes()
    if ref is None:
        raise SystemExit("build oracle/_ref first: make -C oracle ref")
    rng = np.random.default_rng(11)
    k, n = 37, 20000
    boxes = np.concatenate([rng.uniform(-40, 40, (k, 2)), rng.uniform(-1, 1, (k, 1)), rng.uniform(0.5, 6, (k, 3)),
                            rng.uniform(-3.2, 3.2, (k, 1))], 1).astype(np.float32)
    pts = np.concatenate([rng.uniform(-45, 45, (n, 2)), rng.uniform(-3, 3, (n, 1))], 1).astype(np.float32)
    for i in range(k):                                                  # points on / next to every face, incl. the 1e-2 margin shell
        b = boxes[i]
        c, s = np.cos(b[6]), np.sin(b[6])
        for j, (fx, fy, fz) in enumerate([(0.5, 0, 0), (0.5 + 0.01 / b[3], 0, 0), (0, 0.5 + 0.0099 / b[4], 0), (0, 0, 0.5), (0, 0, 0.50001),
                                          (0.499, 0.499, -0.5)]):
            lx, ly, lz = fx * b[3], fy * b[4], fz * b[5]
            pts[i * 6 + j] = [lx * c - ly * s + b[0], lx * s + ly * c + b[1], lz + b[2]]
    mask = ref(boxes, pts)
    extra = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    discard = rng.integers(0, 2, k).astype(bool)
    np.savez_compressed(os.path.join(HERE, "points_in_boxes.npz"), boxes=boxes, points=pts, mask=np.asarray(mask).astype(np.int32),
                        extra=extra, discard=discard)
    print("points_in_boxes: %d boxes x %d points, %d inside" % (k, n, int(np.asarray(mask).sum())))


def merge_sweeps_fixture(m):
    """get_frame's multi-sweep merge and points_rigid_transform (waymo_unsupervised_dataset.py:192-202, 333-360) run from the
    reference file itself: both methods are cut out of the file at generation time and called on a stand-in dataset object that
    serves four sweeps and their poses (eval mode, no annotations: the label branches are not entered; prepare_data returns its
    input). `np.mat` (removed in NumPy 2) is np.asmatrix, as it was in the reference's NumPy. Own RNG."""
    import ast
    import copy
    import textwrap
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    path = os.path.join(REF, "cpd/datasets/waymo_unsupervised/waymo_unsupervised_dataset.py")
    src = open(path).read()
    fns = {n.name: n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef)}
    ns = {"np": np, "copy": copy}
    for name in ("points_rigid_transform", "get_frame"):
        exec(textwrap.dedent(ast.get_source_segment(src, fns[name])), ns)
    rng = np.random.default_rng(333)

    def pose(yaw, t):
        p = np.eye(4)
        p[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        p[:3, 3] = t
        return p

    poses = [pose(0.3 + 0.01 * i, [1200.5 + 1.7 * i, -830.25 + 0.4 * i, 12.0 + 0.02 * i]) for i in range(4)]
    sweeps = [np.concatenate([rng.uniform(-75, 75, (n, 2)), rng.uniform(-2, 4, (n, 1)), rng.uniform(0, 1, (n, 3))], 1).astype(np.float32)
              for n in (5000, 0, 3333, 4097)]
    infos = [{"point_cloud": {"lidar_sequence": "seq", "sample_idx": i}, "pose": poses[i], "frame_id": "f%d" % i} for i in range(4)]
    captured = {}

    class Stand:
        num_data_frames = 4
        all_infos = infos
        training = False
        dataset_cfg = AttrDict(current_label_method="none", labeling_method={})

        def get_lidar(self, seq, idx):
            return sweeps[idx].copy()

        def prepare_data(self, data_dict):
            captured["points"] = np.array(data_dict["points"])       # as merged, before get_frame zeroes columns 3.. at its end
            return dict(data_dict)

    Stand.points_rigid_transform = ns["points_rigid_transform"]
    Stand.get_frame = ns["get_frame"]
    dd = Stand().get_frame(3)
    out = {"merged": captured["points"], "final_points": np.array(dd["points"]), "poses": np.stack(poses)}
    for i, s in enumerate(sweeps):
        out["sweep%d" % i] = s
    np.savez_compressed(os.path.join(HERE, "merge_sweeps.npz"), **out)
    print("merge_sweeps: %s merged rows" % (captured["points"].shape,))


def _randomize_bn(mods, gen):
    with torch.no_grad():
        for mod in mods:
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=gen) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=gen) + 0.5)
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=gen) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=gen) * 0.2)


def wide_dense(m):
    """BaseBEVBackbone / shared conv + SeparateHead at channel widths that are multiples of 32 / 64, so that the split-operand
    workgroup and window kernels (the ones the benchmark runs) can execute these reference goldens; the `bev_backbone` /
    `center_head` fixtures above have 16-channel layers those kernels do not take. Own generator: moves no other fixture."""
    gen = torch.Generator().manual_seed(6464)
    cfg = AttrDict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[64, 128],
                   UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[64, 64])
    torch.manual_seed(6464)
    net = m["bev"].BaseBEVBackbone(cfg, num_frames=1, input_channels=64)
    _randomize_bn(net.modules(), gen)
    net.eval()
    x = torch.randn(2, 64, 24, 20, generator=gen)
    with torch.no_grad():
        y = net({"spatial_features": x})["st_features_2d"]
    d = {"bev_in": x.numpy(), "bev_out": y.numpy(), "layer_nums": np.asarray(cfg.LAYER_NUMS)}
    for k, v in net.state_dict().items():
        d["sd." + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "bev_backbone_wide.npz"), **d)

    head_dict = {"center": dict(out_channels=2, num_conv=2), "center_z": dict(out_channels=1, num_conv=2),
                 "dim": dict(out_channels=3, num_conv=2), "rot": dict(out_channels=2, num_conv=2),
                 "hm": dict(out_channels=3, num_conv=2)}
    sep = m["center_head"].SeparateHead(input_channels=64, sep_head_dict=head_dict, init_bias=-2.19, use_bias=True)
    shared = torch.nn.Sequential(torch.nn.Conv2d(128, 64, 3, stride=1, padding=1, bias=True),
                                 torch.nn.BatchNorm2d(64), torch.nn.ReLU())   # center_head.py:73-80
    _randomize_bn(list(sep.modules()) + list(shared.modules()), gen)
    sep.eval(); shared.eval()
    xh = torch.randn(2, 128, 20, 24, generator=gen)
    with torch.no_grad():
        mid = shared(xh)
        heads = sep(mid)
    d = {"head_in": xh.numpy(), "shared_out": mid.numpy()}
    for k, v in heads.items():
        d["out." + k] = v.numpy()
    for k, v in shared.state_dict().items():
        d["shared." + k] = v.numpy()
    for k, v in sep.state_dict().items():
        d["sep." + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "center_head_wide.npz"), **d)
    print("wide_dense: bev out %s, head maps %s" % (tuple(y.shape), {k: tuple(v.shape) for k, v in heads.items()}))


def main():
    torch.manual_seed(0)
    rng = np.random.default_rng(20240928)
    m = setup_reference()
    if len(sys.argv) > 1 and sys.argv[1] == "nms_large":      # only this (independent) section
        return nms_large(m)
    if len(sys.argv) > 1 and sys.argv[1] == "wide_dense":
        return wide_dense(m)
    if len(sys.argv) > 1 and sys.argv[1] == "atss":
        return atss(m)
    if len(sys.argv) > 1 and sys.argv[1] == "proto_crop":
        return proto_crop(m)
    if len(sys.argv) > 1 and sys.argv[1] == "proto_head":
        return proto_head(m)
    if len(sys.argv) > 1 and sys.argv[1] == "target_layer_x":
        return target_layer_x(m)
    if len(sys.argv) > 1 and sys.argv[1] == "points_in_boxes":
        return points_in_boxes_fixture(m)
    if len(sys.argv) > 1 and sys.argv[1] == "merge_sweeps":
        return merge_sweeps_fixture(m)
    lib = m["lib"]
    out = {}

    # ---- 1. MeanVFE (mean_vfe.py:16-61) ------------------------------------------------------
    M, P, C = 257, 5, 5
    num = rng.integers(0, P + 1, M).astype(np.int32)
    vox = rng.normal(0, 3, (M, P, C)).astype(np.float32)
    for v in range(M):
        vox[v, num[v]:] = 0
    vfe = m["mean_vfe"].MeanVFE(AttrDict(), num_point_features=C, num_frames=1)
    bd = {"voxels": torch.from_numpy(vox), "voxel_num_points": torch.from_numpy(num)}
    feat = vfe(bd)["voxel_features"].numpy()
    np.savez_compressed(os.path.join(HERE, "mean_vfe.npz"), voxels=vox, num_points=num, features=feat)

    # ---- 2. BaseBEVBackbone (base_bev_backbone.py:6-122), reduced widths ---------------------
    cfg = AttrDict(LAYER_NUMS=[2, 2], LAYER_STRIDES=[1, 2], NUM_FILTERS=[16, 32],
                   UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[32, 32])
    net = m["bev"].BaseBEVBackbone(cfg, num_frames=1, input_channels=32)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.3)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.2)
    net.eval()
    x = torch.randn(1, 32, 24, 20)
    with torch.no_grad():
        y = net({"spatial_features": x})["st_features_2d"]
    d = {"bev_in": x.numpy(), "bev_out": y.numpy()}
    for k, v in net.state_dict().items():
        d["sd." + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "bev_backbone.npz"), **d)

    # ---- 3. shared conv + SeparateHead (center_head.py:11-45,73-80) --------------------------
    head_dict = {"center": dict(out_channels=2, num_conv=2), "center_z": dict(out_channels=1, num_conv=2),
                 "dim": dict(out_channels=3, num_conv=2), "rot": dict(out_channels=2, num_conv=2),
                 "hm": dict(out_channels=3, num_conv=2)}
    sep = m["center_head"].SeparateHead(input_channels=16, sep_head_dict=head_dict, init_bias=-2.19, use_bias=True)
    shared = torch.nn.Sequential(torch.nn.Conv2d(64, 16, 3, stride=1, padding=1, bias=True),
                                 torch.nn.BatchNorm2d(16), torch.nn.ReLU())   # center_head.py:73-80
    with torch.no_grad():
        for mod in list(sep.modules()) + list(shared.modules()):
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.3)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.2)
    sep.eval(); shared.eval()
    xh = torch.randn(1, 64, 20, 24)
    with torch.no_grad():
        mid = shared(xh)
        heads = sep(mid)
    d = {"head_in": xh.numpy(), "shared_out": mid.numpy()}
    for k, v in heads.items():
        d["out." + k] = v.numpy()
    for k, v in shared.state_dict().items():
        d["shared." + k] = v.numpy()
    for k, v in sep.state_dict().items():
        d["sep." + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "center_head.npz"), **d)

    # ---- 4. _topk + decode_bbox_from_heatmap (centernet_utils.py:136-216) ---------------------
    cu = m["centernet_utils"]
    H, W, K = 47, 47, 60
    hm_logit = torch.randn(1, 3, H, W) * 1.5 - 1.0
    center = torch.randn(1, 2, H, W) * 0.3
    center_z = torch.randn(1, 1, H, W) * 0.5
    dim_log = torch.randn(1, 3, H, W) * 0.3 + 0.8
    rot = torch.randn(1, 2, H, W)
    pcr = [-75.2, -75.2, -2, 75.2, 75.2, 4]
    vs = [0.1, 0.1, 0.15]
    stride = 32  # 47*32*0.1 = 150.4 m span
    limit = torch.tensor([-70.0, -70.0, -1.0, 70.0, 70.0, 1.0])
    ts, ti, tc, ty, tx = cu._topk(hm_logit.sigmoid(), K=K)
    dec = cu.decode_bbox_from_heatmap(
        heatmap=hm_logit.sigmoid(), rot_cos=rot[:, 0:1], rot_sin=rot[:, 1:2], center=center,
        center_z=center_z, dim=dim_log.exp(), point_cloud_range=pcr, voxel_size=vs,
        feature_map_stride=stride, K=K, circle_nms=False, score_thresh=0.1,
        post_center_limit_range=limit)[0]
    np.savez_compressed(
        os.path.join(HERE, "decode.npz"), hm=hm_logit.numpy(), center=center.numpy(),
        center_z=center_z.numpy(), dim=dim_log.numpy(), rot=rot.numpy(), K=K, stride=stride,
        pcr=np.array(pcr, np.float32), vs=np.array(vs, np.float32), limit=limit.numpy(), score_thresh=0.1,
        topk_scores=ts.numpy(), topk_inds=ti.numpy(), topk_classes=tc.numpy(), topk_ys=ty.numpy(),
        topk_xs=tx.numpy(), boxes=dec["pred_boxes"].numpy(), scores=dec["pred_scores"].numpy(),
        labels=dec["pred_labels"].numpy())

    # ---- 5. BEV IoU matrices from the compiled reference iou3d_cpu.cpp ------------------------
    a = rand_boxes(rng, 150, span=12.0)
    b = rand_boxes(rng, 130, span=12.0)
    adv = adversarial_boxes(rng)
    np.savez_compressed(os.path.join(HERE, "iou_bev.npz"), a=a, b=b, iou_ab=ref_iou_bev(lib, a, b),
                        adv=adv, iou_adv=ref_iou_bev(lib, adv, adv))

    # ---- 6. class_agnostic_nms (model_nms_utils.py:115-134) -----------------------------------
    d = {}
    for tag, n, thr, span in [("n64", 64, 0.8, 8.0), ("n500", 500, 0.8, 25.0), ("n500_t3", 500, 0.3, 25.0),
                              ("n1000_t1", 1000, 0.1, 40.0)]:
        for attempt in range(400):
            bx = rand_boxes(rng, n, span=span)
            k = n // 10
            bx[n - k:] = bx[:k]
            bx[n - k:, :2] += rng.normal(0, 0.25, (k, 2)).astype(np.float32)
            bx[n - k:, 6] += rng.normal(0, 0.05, k).astype(np.float32)
            sc = rng.permutation(n).astype(np.float32) / n + 0.001  # distinct scores
            order = np.argsort(-sc, kind="stable")
            iou = ref_iou_bev(lib, bx[order], bx[order])
            if borderline_free(iou[np.triu_indices(n, 1)], thr):
                break
        else:
            raise RuntimeError("no borderline-free set for " + tag)
        cfgn = AttrDict(NMS_TYPE="nms_gpu", NMS_THRESH=thr, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500)
        sel, sel_sc = m["model_nms_utils"].class_agnostic_nms(
            box_scores=torch.from_numpy(sc), box_preds=torch.from_numpy(bx), nms_config=cfgn, score_thresh=None)
        d[tag + ".boxes"] = bx
        d[tag + ".scores"] = sc
        d[tag + ".thr"] = np.float32(thr)
        d[tag + ".selected"] = sel.numpy()
        d[tag + ".selected_scores"] = sel_sc.numpy()
    np.savez_compressed(os.path.join(HERE, "nms.npz"), **d)

    # ---- 7. CenterHead target assignment + losses (center_head.py:103-250, loss_utils.py:265-386) -----
    ch = m["center_head"]
    fake_self = types.SimpleNamespace(point_cloud_range=[-75.2, -75.2, -2, 75.2, 75.2, 4], voxel_size=[0.1, 0.1, 0.15])
    n_gt = 40
    gt = torch.zeros(n_gt, 8)
    gt[:, 0:2] = torch.from_numpy(rng.uniform(-70, 70, (n_gt, 2))).float()
    gt[:, 2] = torch.from_numpy(rng.uniform(-1, 1, n_gt)).float()
    sizes = torch.tensor([[5.065, 1.86, 1.49], [1.0, 1.0, 2.0], [1.9, 0.85, 1.8]])
    cls = torch.from_numpy(rng.integers(1, 4, n_gt))
    gt[:, 3:6] = sizes[cls - 1] * torch.from_numpy(rng.uniform(0.9, 1.1, (n_gt, 3))).float()
    gt[:, 6] = torch.from_numpy(rng.uniform(-np.pi, np.pi, n_gt)).float()
    gt[:, 7] = cls.float()
    gt[:3, 0:2] = torch.tensor([[75.19, -75.19], [-75.2, 75.19], [0.03, 0.04]])       # border / clamped centres
    heat, ret_boxes, inds, mask = ch.CenterHead.assign_target_of_single_head(
        fake_self, num_classes=3, gt_boxes=gt.clone(), feature_map_size=[188, 188], feature_map_stride=8,
        num_max_objs=500, gaussian_overlap=0.1, min_radius=2)
    lu = m["loss_utils"]
    pred_hm = torch.clamp(torch.randn(2, 3, 24, 20).sigmoid(), 1e-4, 1 - 1e-4)
    gt_hm = torch.rand(2, 3, 24, 20) ** 4
    gt_hm.view(-1)[torch.randperm(gt_hm.numel())[:25]] = 1.0
    focal = lu.FocalLossCenterNet()(pred_hm, gt_hm)
    reg_out = torch.randn(2, 8, 24, 20)
    reg_inds = torch.randint(0, 24 * 20, (2, 50))
    reg_mask = (torch.rand(2, 50) > 0.4).long()
    reg_tgt = torch.randn(2, 50, 8)
    regl = lu.RegLossCenterNet()(reg_out, reg_mask, reg_inds, reg_tgt)
    np.savez_compressed(os.path.join(HERE, "center_loss.npz"), gt_boxes=gt.numpy(), heatmap=heat.numpy(),
                        ret_boxes=ret_boxes.numpy(), inds=inds.numpy(), mask=mask.numpy(), pred_hm=pred_hm.numpy(),
                        gt_hm=gt_hm.numpy(), focal=focal.numpy(), reg_out=reg_out.numpy(), reg_inds=reg_inds.numpy(),
                        reg_mask=reg_mask.numpy(), reg_tgt=reg_tgt.numpy(), reg_loss=regl.numpy())
    # 8. RoI-head feature pooling: the reference's NeighborVoxelSAModuleMSG /
    #    VoxelQueryAndGrouping / GroupingOperation Python (voxel_pool_modules.py, voxel_query_utils.py,
    #    pointnet2_utils.py), get_global_grid_points_of_roi and get_voxel_centers, with the CUDA extension
    #    pointnet2_stack_cuda replaced by the oracle's restatement of its two kernels (oracle/cpd_oracle.c;
    #    those kernels themselves cannot be executed here) and torch.cuda.*Tensor mapped to CPU tensors.
    sys.path.insert(0, REPO)
    from oracle.binding import Oracle
    orc = Oracle()
    for pkg in ["r.ops.pointnet2", "r.ops.pointnet2.pointnet2_stack", "r.models.roi_heads"]:
        _pkg(pkg)
    ext = types.ModuleType("r.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda")

    def voxel_query_wrapper(M, Z, Y, X, nsample, radius, zr, yr, xr, new_xyz, xyz, new_coords, point_indices, idx):
        idx.copy_(torch.from_numpy(orc.voxel_query([zr, yr, xr], radius, nsample, xyz.numpy(), new_xyz.numpy(),
                                                   new_coords.numpy(), point_indices.numpy())))

    def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, output):
        output.copy_(torch.from_numpy(orc.group_points(features.detach().numpy(), features_batch_cnt.numpy(), idx.numpy(),
                                                       idx_batch_cnt.numpy())))

    ext.voxel_query_wrapper, ext.group_points_wrapper = voxel_query_wrapper, group_points_wrapper
    sys.modules[ext.__name__] = ext
    sys.modules["r.ops.pointnet2.pointnet2_stack"].pointnet2_stack_cuda = ext
    torch.cuda.IntTensor = lambda *sz: torch.zeros(*sz, dtype=torch.int32)
    torch.cuda.FloatTensor = lambda *sz: torch.zeros(*sz, dtype=torch.float32)
    pu = _load("r.ops.pointnet2.pointnet2_stack.pointnet2_utils", "cpd/ops/pointnet2/pointnet2_stack/pointnet2_utils.py")
    sys.modules["r.ops.pointnet2.pointnet2_stack"].pointnet2_utils = pu
    vq = _load("r.ops.pointnet2.pointnet2_stack.voxel_query_utils", "cpd/ops/pointnet2/pointnet2_stack/voxel_query_utils.py")
    sys.modules["r.ops.pointnet2.pointnet2_stack"].voxel_query_utils = vq
    vp = _load("r.ops.pointnet2.pointnet2_stack.voxel_pool_modules", "cpd/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py")

    torch.manual_seed(21)
    g = np.random.default_rng(21)
    B, shape, stride = 2, [6, 40, 44], 4                      # an x_conv3-like level: (Z, Y, X), stride 4
    vsz, pcr = [0.1, 0.1, 0.15], [-8.8, -8.0, -2.0, 8.8, 8.0, 1.6]
    cells = np.unique(np.stack([g.integers(0, B, 2600), g.integers(0, shape[0], 2600), g.integers(0, shape[1], 2600),
                                g.integers(0, shape[2], 2600)], 1), axis=0).astype(np.int32)       # canonical (b,z,y,x) order
    feats = torch.randn(cells.shape[0], 16)
    # voxel centres as voxel_rcnn_head.py:231-236 computes them (common_utils.get_voxel_centers, l.66-82)
    vc = torch.from_numpy(cells[:, [3, 2, 1]].astype(np.float32))
    xyz = (vc + 0.5) * (torch.tensor(vsz) * stride) + torch.tensor(pcr[:3])
    xyz_cnt = torch.tensor([(cells[:, 0] == b).sum() for b in range(B)], dtype=torch.int32)
    # rois and their 3x3x3 grid points (voxel_rcnn_head.py:365-386, common_utils.rotate_points_along_z)
    rois = torch.tensor(np.concatenate([g.uniform(-6, 6, (B, 7, 2)), g.uniform(-1.2, 0.8, (B, 7, 1)),
                                        g.uniform(1.0, 4.5, (B, 7, 3)), g.uniform(-3.1, 3.1, (B, 7, 1))], -1), dtype=torch.float32)
    GS = 3
    flat = rois.view(-1, 7)
    dense_idx = torch.ones(GS, GS, GS).nonzero().repeat(flat.shape[0], 1, 1).float()
    local = (dense_idx + 0.5) / GS * flat[:, None, 3:6] - flat[:, None, 3:6] / 2
    ca, sa = torch.cos(flat[:, 6]), torch.sin(flat[:, 6])
    rot = torch.stack([ca, sa, torch.zeros_like(ca), -sa, ca, torch.zeros_like(ca), torch.zeros_like(ca), torch.zeros_like(ca),
                       torch.ones_like(ca)], 1).view(-1, 3, 3)
    grid_xyz = (torch.matmul(local, rot) + flat[:, None, 0:3]).view(B, -1, 3)                      # (B, N*27, 3)
    gc = torch.cat([(grid_xyz[..., 0:1] - pcr[0]) // vsz[0], (grid_xyz[..., 1:2] - pcr[1]) // vsz[1],
                    (grid_xyz[..., 2:3] - pcr[2]) // vsz[2]], -1)                                  # l.207-211
    bidx = torch.arange(B, dtype=torch.float32).view(B, 1, 1).expand(B, gc.shape[1], 1)
    new_coords = torch.cat([bidx, gc // stride], -1).int().view(-1, 4)                             # l.243-245, (b, x, y, z)
    new_cnt = torch.full((B,), gc.shape[1], dtype=torch.int32)
    v2p = torch.from_numpy(orc.voxel2pinds(cells, B, shape))
    mod = vp.NeighborVoxelSAModuleMSG(query_ranges=[[1, 2, 2], [2, 4, 4]], radii=[0.9, 1.7], nsamples=[8, 16],
                                      mlps=[[16, 16, 24], [16, 16, 24]], pool_method="max_pool").eval()
    for mm in mod.modules():
        if isinstance(mm, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            mm.weight.data.uniform_(0.6, 1.4); mm.bias.data.normal_(0, 0.2)
            mm.running_mean.normal_(0, 0.2); mm.running_var.uniform_(0.6, 1.4)
    with torch.no_grad():
        pooled = mod(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_cnt, new_xyz=grid_xyz.contiguous().view(-1, 3),
                     new_xyz_batch_cnt=new_cnt, new_coords=new_coords.contiguous(), features=feats.contiguous(),
                     voxel2point_indices=v2p)
        raw_idx, empty = vq.voxel_query([1, 2, 2], 0.9, 8, xyz.contiguous(), grid_xyz.contiguous().view(-1, 3),
                                        new_coords[:, [0, 3, 2, 1]].contiguous(), v2p)
    d = {"sd." + k: v.numpy() for k, v in mod.state_dict().items()}
    d.update(cells=cells, shape=np.array(shape), stride=stride, voxel_size=np.array(vsz, np.float32), pcr=np.array(pcr, np.float32),
             feats=feats.numpy(), xyz=xyz.numpy(), rois=rois.numpy(), grid_size=GS, grid_xyz=grid_xyz.numpy(),
             new_coords_bxyz=new_coords.numpy(), pooled=pooled.numpy(), query_idx=raw_idx.numpy(), query_empty=empty.numpy())
    np.savez_compressed(os.path.join(HERE, "roi_pool.npz"), **d)
    print("roi_pool: %d voxels, %d grid points, %d empty balls (range 0)" % (cells.shape[0], new_coords.shape[0], int(empty.sum())))
    # 9. Anchor head: the reference's own AnchorGenerator, ResidualCoder, box_utils nearest-BEV IoU,
    #    AxisAlignedTargetAssigner.assign_targets and AnchorHeadTemplate.generate_predicted_boxes, all plain torch,
    #    loaded by file path (Tensor.cuda() mapped to identity on this GPU-less box; match_height=False, so the
    #    iou3d_nms stub is never called).
    import types as _t
    from types import SimpleNamespace
    torch.Tensor.cuda = lambda self, *a, **k: self
    for pkg in ["r.models.dense_heads.target_assigner"]:
        _pkg(pkg)
    cu = _load("r.utils.common_utils_real", "cpd/utils/common_utils.py") if False else None
    common = _t.ModuleType("r.utils.common_utils")

    def check_numpy_to_torch(x):
        if isinstance(x, np.ndarray):
            return torch.from_numpy(x).float(), True
        return x, False

    def limit_period(val, offset=0.5, period=np.pi):                   # cpd/utils/common_utils.py:17-20 verbatim semantics
        val, is_numpy = check_numpy_to_torch(val)
        ans = val - torch.floor(val / period + offset) * period
        return ans.numpy() if is_numpy else ans

    common.check_numpy_to_torch, common.limit_period = check_numpy_to_torch, limit_period
    sys.modules["r.utils.common_utils"] = common
    sys.modules["r.utils"].common_utils = common
    for stub in ["r.ops.roiaware_pool3d", "r.ops.roiaware_pool3d.roiaware_pool3d_utils"]:
        sys.modules[stub] = _t.ModuleType(stub)
    sys.modules["r.ops"].roiaware_pool3d = sys.modules["r.ops.roiaware_pool3d"]
    sys.modules["r.ops.roiaware_pool3d"].roiaware_pool3d_utils = sys.modules["r.ops.roiaware_pool3d.roiaware_pool3d_utils"]
    sys.modules["scipy.spatial"] = __import__("scipy.spatial").spatial
    bu = _load("r.utils.box_utils", "cpd/utils/box_utils.py")
    sys.modules["r.utils"].box_utils = bu
    bc = _load("r.utils.box_coder_utils", "cpd/utils/box_coder_utils.py")
    ag = _load("r.models.dense_heads.target_assigner.anchor_generator",
               "cpd/models/dense_heads/target_assigner/anchor_generator.py")
    ta = _load("r.models.dense_heads.target_assigner.axis_aligned_target_assigner",
               "cpd/models/dense_heads/target_assigner/axis_aligned_target_assigner.py")
    g = np.random.default_rng(33)
    torch.manual_seed(33)
    pcr = np.array([-20.8, -20.8, -2.0, 20.8, 20.8, 4.0], np.float32)
    agc = [AttrDict(class_name="Vehicle", anchor_sizes=[[4.7, 2.1, 1.7]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0],
                    align_center=False, feature_map_stride=8, matched_threshold=0.55, unmatched_threshold=0.4),
           AttrDict(class_name="Pedestrian", anchor_sizes=[[0.91, 0.86, 1.73]], anchor_rotations=[0, 1.57],
                    anchor_bottom_heights=[0], align_center=False, feature_map_stride=8, matched_threshold=0.5,
                    unmatched_threshold=0.35),
           AttrDict(class_name="Cyclist", anchor_sizes=[[1.78, 0.84, 1.78]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0],
                    align_center=False, feature_map_stride=8, matched_threshold=0.5, unmatched_threshold=0.35)]
    H = W = 52
    gen = ag.AnchorGenerator(anchor_range=pcr, anchor_generator_config=agc)
    anchors_list, per_loc = gen.generate_anchors([[W, H]] * 3)            # each (1, H, W, 1, 2, 7)
    coder = bc.ResidualCoder()
    n_gt = 14
    cls = g.integers(1, 4, (2, n_gt))
    sizes = np.array([[4.7, 2.1, 1.7], [0.91, 0.86, 1.73], [1.78, 0.84, 1.78]])
    gt = np.zeros((2, n_gt + 3, 8), np.float32)
    for b in range(2):
        for i in range(n_gt):
            gt[b, i] = [g.uniform(-19, 19), g.uniform(-19, 19), g.uniform(-0.5, 0.5), *(sizes[cls[b, i] - 1] * g.uniform(0.85, 1.15, 3)),
                        g.uniform(-3.1, 3.1), cls[b, i]]
    cfg_ta = AttrDict(ANCHOR_GENERATOR_CONFIG=agc, TARGET_ASSIGNER_CONFIG=AttrDict(POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                      NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False))
    assigner = ta.AxisAlignedTargetAssigner(model_cfg=cfg_ta, class_names=["Vehicle", "Pedestrian", "Cyclist"], box_coder=coder,
                                            grid_size=np.array([416, 416, 40]), point_cloud_range=pcr, match_height=False)
    tgt = assigner.assign_targets([a.clone() for a in anchors_list], torch.from_numpy(gt))
    ious = bu.boxes3d_nearest_bev_iou(anchors_list[0].view(-1, 7)[::37], torch.from_numpy(gt[0, :n_gt, :7]))
    enc = coder.encode_torch(torch.from_numpy(gt[0, :n_gt, :7]).clone(), anchors_list[0].view(-1, 7)[:n_gt].clone())
    # generate_predicted_boxes as an unbound call (AnchorHeadTemplate needs .cuda() modules to construct)
    for stub in ["r.models.model_utils.model_nms_utils"]:
        pass
    _load("r.models.dense_heads.target_assigner.atss_target_assigner",
          "cpd/models/dense_heads/target_assigner/atss_target_assigner.py")
    sys.modules["r.utils"].box_coder_utils = bc
    _load("r.utils.odiou_loss", "cpd/utils/odiou_loss.py")            # plain torch/scipy; only constructed, never called here
    aht = _load("r.models.dense_heads.anchor_head_template", "cpd/models/dense_heads/anchor_head_template.py")
    n_loc = H * W
    n_anc = n_loc * 6
    cls_preds = torch.randn(2, H, W, 6 * 3)
    box_preds = torch.randn(2, H, W, 6 * 7) * 0.3
    dir_preds = torch.randn(2, H, W, 6 * 2)
    fake = SimpleNamespace(anchors=[a.clone() for a in anchors_list], use_multihead=False, box_coder=coder,
                           model_cfg=AttrDict(DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2))
    bcp, bbp = aht.AnchorHeadTemplate.generate_predicted_boxes(fake, 2, cls_preds, box_preds, dir_preds)
    np.savez_compressed(os.path.join(HERE, "anchor_head.npz"), pcr=pcr, hw=np.array([H, W]),
                        anchors=torch.cat(anchors_list, dim=-3).numpy(), anchors_per_class=torch.stack(anchors_list).numpy(),
                        gt=gt, labels=tgt["box_cls_labels"].numpy(), reg_targets=tgt["box_reg_targets"].numpy(),
                        reg_weights=tgt["reg_weights"].numpy(), gt_ious=tgt["gt_ious"].numpy(), iou_sample=ious.numpy(),
                        enc=enc.numpy(), cls_preds=cls_preds.numpy(), box_preds=box_preds.numpy(), dir_preds=dir_preds.numpy(),
                        decoded=bbp.numpy(), batch_cls=bcp.numpy())
    # 10. AnchorHeadSingle.forward in eval mode (anchor_head_single.py:194-356), constructed on CPU thanks to the
    #     identity Tensor.cuda: occupancy anchor mask (l.238-278, incl. its wrap-around negative indices), the three
    #     1x1 convs, masked anchors, generate_predicted_boxes.
    sys.modules["r.models.model_utils"].model_nms_utils = m["model_nms_utils"]
    sys.modules.setdefault("cv2", _t.ModuleType("cv2"))              # imported by the reference file (l.6), never used
    ahs = _load("r.models.dense_heads.anchor_head_single", "cpd/models/dense_heads/anchor_head_single.py")
    mcfg = AttrDict(ANCHOR_GENERATOR_CONFIG=agc, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
                    TARGET_ASSIGNER_CONFIG=AttrDict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                                    NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER="ResidualCoder"),
                    LOSS_CONFIG=AttrDict(LOSS_WEIGHTS=AttrDict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2,
                                                               code_weights=[1.0] * 7)))
    head = ahs.AnchorHeadSingle(model_cfg=mcfg, num_frames=1, input_channels=24, num_class=3, class_names=["Vehicle", "Pedestrian", "Cyclist"],
                                grid_size=np.array([416, 416, 40]), point_cloud_range=pcr, predict_boxes_when_training=False).eval()
    with torch.no_grad():
        head.conv_box.weight.normal_(0, 0.05); head.conv_cls.weight.normal_(0, 0.05); head.conv_dir_cls.weight.normal_(0, 0.05)
    pts_bev = torch.cat([torch.zeros(300, 1), torch.from_numpy(g.uniform(-20.5, 20.5, (300, 3)).astype(np.float32))], 1)
    pts_bev[:150, 1:3] *= 0.35                                        # a cluster, so the mask is neither empty nor full
    pts_bev = pts_bev[(pts_bev[:, 1].abs() < 9) | (pts_bev[:, 2] > 12)]
    feat2d = torch.randn(2, 24, H, W)
    dd = {"points": pts_bev, "st_features_2d": feat2d, "batch_size": 2}
    with torch.no_grad():
        mask = head.get_anchor_mask(dd, feat2d.shape)
        outd = head(dict(dd))
    ah_sd = {"ahs." + k: v.numpy() for k, v in head.state_dict().items()}
    np.savez_compressed(os.path.join(HERE, "anchor_head_single.npz"), points=pts_bev.numpy(), feat=feat2d.numpy(), mask=mask.numpy(),
                        batch_cls_preds=outd["batch_cls_preds"].numpy(), batch_box_preds=outd["batch_box_preds"].numpy(), pcr=pcr, **ah_sd)
    # 12. AnchorHeadTemplate.get_loss (anchor_head_template.py:179-334) on the real AnchorHeadSingle object of section 10,
    #     fed with section 9's predictions and assigned targets: SigmoidFocalClassificationLoss, WeightedSmoothL1Loss with the
    #     sin-difference encoding, WeightedCrossEntropyLoss on the direction bins (loss_utils.py:10-206), and the gradients
    #     autograd gives w.r.t. the three prediction maps (every 5th anchor + whole-tensor sums, to keep the fixture small).
    lp = [t.clone().requires_grad_(True) for t in (cls_preds, box_preds, dir_preds)]
    # a fresh head (section 10's eval forward left its occupancy-masked anchors in head.anchors) with the full anchor set
    head = ahs.AnchorHeadSingle(model_cfg=mcfg, num_frames=1, input_channels=24, num_class=3, class_names=["Vehicle", "Pedestrian", "Cyclist"],
                                grid_size=np.array([416, 416, 40]), point_cloud_range=pcr, predict_boxes_when_training=False)
    head.train()
    head.anchors = [a.clone() for a in head.anchors_root]      # what forward() installs when no anchor is masked out
    head.forward_ret_dict = {"cls_preds": lp[0], "box_preds": lp[1], "dir_cls_preds": lp[2],
                             "box_cls_labels": tgt["box_cls_labels"].clone(), "box_reg_targets": tgt["box_reg_targets"].clone()}
    rpn_loss, tb = head.get_loss()
    rpn_loss.backward()
    gl = [t.grad.reshape(2, n_anc, -1) for t in lp]
    np.savez_compressed(os.path.join(HERE, "anchor_loss.npz"), rpn_loss=np.float32(rpn_loss.item()),
                        cls_loss=np.float32(tb["rpn_loss_cls"]), loc_loss=np.float32(tb["rpn_loss_loc"]), dir_loss=np.float32(tb["rpn_loss_dir"]),
                        weights=np.array([1.0, 2.0, 0.2], np.float32), dir_offset=np.float32(0.78539),
                        g_cls=gl[0][:, ::5].numpy(), g_box=gl[1][:, ::5].numpy(), g_dir=gl[2][:, ::5].numpy(),
                        g_sums=np.array([[g_.sum().item(), g_.abs().sum().item()] for g_ in gl], np.float64))
    print("anchor_loss: rpn %.6f = cls %.6f + loc %.6f + dir %.6f" % (rpn_loss.item(), tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb["rpn_loss_dir"]))
    # 11. VoxelRCNNHead eval forward (voxel_rcnn_head.py:664-760, 876-916; roi_head_template.py:269-299): RoI grid
    #     pooling on two levels, shared FC / cls / reg layers, box decoding in the RoI frame. The real common_utils.py
    #     and spconv_utils.py are loaded by file; pointnet2_stack_cuda stays the oracle-backed stub of section 8.
    cu_real = _load("r.utils.common_utils", "cpd/utils/common_utils.py")
    sys.modules["r.utils"].common_utils = cu_real
    su = _load("r.utils.spconv_utils_probe", "cpd/utils/spconv_utils.py") if False else None
    spu = _t.ModuleType("r.utils.spconv_utils")                       # generate_voxel2pinds only (the file imports spconv at top)

    def generate_voxel2pinds(sparse_tensor):                            # cpd/utils/spconv_utils.py:4-21 semantics on the oracle
        return torch.from_numpy(orc.voxel2pinds(sparse_tensor.indices.numpy().astype(np.int32), sparse_tensor.batch_size,
                                                list(sparse_tensor.spatial_shape)))

    spu.generate_voxel2pinds = generate_voxel2pinds
    sys.modules["r.utils.spconv_utils"] = spu
    sys.modules["r.utils"].spconv_utils = spu
    for pkg in ["r.models.roi_heads.target_assigner"]:
        _pkg(pkg)
    _load("r.utils.bbloss", "cpd/utils/bbloss.py")
    _load("r.models.roi_heads.target_assigner.proposal_target_layer", "cpd/models/roi_heads/target_assigner/proposal_target_layer.py")
    _load("r.models.roi_heads.roi_head_template", "cpd/models/roi_heads/roi_head_template.py")
    sys.modules["r.ops.pointnet2"].pointnet2_stack = sys.modules["r.ops.pointnet2.pointnet2_stack"]
    sys.modules["r.ops.pointnet2.pointnet2_stack"].voxel_pool_modules = vp
    vrh = _load("r.models.roi_heads.voxel_rcnn_head", "cpd/models/roi_heads/voxel_rcnn_head.py")
    rcfg = AttrDict(
        ROI_GRID_POOL=AttrDict(FEATURES_SOURCE=["x_conv3", "x_conv4"], PRE_MLP=True, GRID_SIZE=3, POOL_LAYERS=AttrDict(
            x_conv3=AttrDict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[0.6, 1.2], NSAMPLE=[8, 8],
                             POOL_METHOD="max_pool"),
            x_conv4=AttrDict(MLPS=[[16, 16], [16, 16]], QUERY_RANGES=[[1, 1, 1], [2, 2, 2]], POOL_RADIUS=[1.2, 2.4], NSAMPLE=[8, 8],
                             POOL_METHOD="max_pool"))),
        SHARED_FC=[64, 64], CLS_FC=[32], REG_FC=[32], DP_RATIO=0.3,
        TARGET_CONFIG=AttrDict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=16, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                               CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
                               HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55),
        LOSS_CONFIG=AttrDict(LOSS_WEIGHTS=AttrDict(code_weights=[1.0] * 7)),
        NMS_CONFIG=AttrDict(TEST=AttrDict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=100,
                                          NMS_THRESH=0.7)))
    torch.manual_seed(41)
    rhead = vrh.VoxelRCNNHead(input_channels={"x_conv3": 24, "x_conv4": 32}, model_cfg=rcfg, point_cloud_range=pcr,
                              voxel_size=[0.1, 0.1, 0.15], num_class=1).eval()
    for mm in rhead.modules():
        if isinstance(mm, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            mm.weight.data.uniform_(0.6, 1.4); mm.bias.data.normal_(0, 0.2)
            mm.running_mean.normal_(0, 0.2); mm.running_var.uniform_(0.6, 1.4)
    with torch.no_grad():
        rhead.cls_layers[-1].weight.normal_(0, 0.1); rhead.reg_layers[-1].weight.normal_(0, 0.05)
    lv = {}
    for name, shp, stride_l, ch, nvox in (("x_conv3", [11, 104, 104], 4, 24, 5000), ("x_conv4", [5, 52, 52], 8, 32, 2200)):
        cl = np.unique(np.stack([g.integers(0, 2, nvox), g.integers(0, shp[0], nvox), g.integers(0, shp[1], nvox),
                                 g.integers(0, shp[2], nvox)], 1), axis=0).astype(np.int32)
        lv[name] = SimpleNamespace(indices=torch.from_numpy(cl), features=torch.randn(cl.shape[0], ch), spatial_shape=shp, batch_size=2)
    rois_in = torch.tensor(np.concatenate([g.uniform(-18, 18, (2, 9, 2)), g.uniform(-0.5, 1.0, (2, 9, 1)), g.uniform(1.0, 4.5, (2, 9, 3)),
                                           g.uniform(-3.1, 3.1, (2, 9, 1))], -1), dtype=torch.float32)
    bd = {"batch_size": 2, "rois": rois_in.clone(), "roi_labels": torch.ones(2, 9).long(), "multi_scale_3d_features": lv,
          "multi_scale_3d_strides": {"x_conv3": 4, "x_conv4": 8}}
    with torch.no_grad():
        od = rhead(bd)
    rsd = {"rh." + k: v.numpy() for k, v in rhead.state_dict().items()}
    np.savez_compressed(os.path.join(HERE, "voxel_rcnn_head.npz"), rois=rois_in.numpy(), pcr=pcr,
                        c3_idx=lv["x_conv3"].indices.numpy(), c3_feat=lv["x_conv3"].features.numpy(),
                        c4_idx=lv["x_conv4"].indices.numpy(), c4_feat=lv["x_conv4"].features.numpy(),
                        batch_cls_preds=od["batch_cls_preds"].numpy(), batch_box_preds=od["batch_box_preds"].numpy(), **rsd)
    print("voxel_rcnn_head: %d rois -> cls %s box %s" % (rois_in.shape[0] * rois_in.shape[1], tuple(od["batch_cls_preds"].shape),
                                                          tuple(od["batch_box_preds"].shape)))
    print("anchor_head_single: mask keeps %d of %d locations, %d boxes/sample" % (int(mask.sum()), mask.numel(), outd["batch_box_preds"].shape[1]))
    print("anchor_head: %d anchors, %d positives, %d ignored" % (n_anc, int((tgt["box_cls_labels"] > 0).sum()),
                                                                  int((tgt["box_cls_labels"] < 0).sum())))
    # 13. AnchorHeadSingleV2.forward in eval mode (anchor_head_single.py:9-29,31-192) -- the head both shipped dbscan / oyster
    #     configs select: shared 3x3 conv + BN + ReLU, five get_layer branches (3x3 conv + BN + ReLU + 1x1 conv), the 1x1
    #     direction classifier on the input map, occupancy-masked anchors, generate_predicted_boxes. Own generators: this
    #     section moves no other fixture.
    gen2 = torch.Generator().manual_seed(2222)
    g2 = np.random.default_rng(2222)
    torch.manual_seed(2222)
    head2 = ahs.AnchorHeadSingleV2(model_cfg=mcfg, num_frames=1, input_channels=32, num_class=3,
                                   class_names=["Vehicle", "Pedestrian", "Cyclist"], grid_size=np.array([416, 416, 40]),
                                   point_cloud_range=pcr, predict_boxes_when_training=False).eval()
    with torch.no_grad():
        for name, prm in head2.named_parameters():                   # the reference's init (std 0.001) would hide layout mistakes
            if prm.dim() == 4:
                prm.copy_(torch.randn(prm.shape, generator=gen2) * (2.0 / (prm.shape[1] * prm.shape[2] * prm.shape[3])) ** 0.5)
            elif "bias" in name and prm.numel() > 1 and not name.endswith("3.bias"):
                prm.copy_(torch.randn(prm.shape, generator=gen2) * 0.1)
        _randomize_bn(head2.modules(), gen2)
    pts2 = torch.cat([torch.zeros(260, 1), torch.from_numpy(g2.uniform(-20.5, 20.5, (260, 3)).astype(np.float32))], 1)
    pts2[:120, 1:3] *= 0.4
    pts2 = pts2[(pts2[:, 1].abs() < 10) | (pts2[:, 2] > 11)]
    feat2 = torch.randn(2, 32, H, W, generator=gen2)
    dd2 = {"points": pts2, "st_features_2d": feat2, "batch_size": 2}
    with torch.no_grad():
        mask2 = head2.get_anchor_mask(dd2, feat2.shape)
        out2 = head2(dict(dd2))
    sd2 = {"v2." + k: v.numpy() for k, v in head2.state_dict().items()}
    np.savez_compressed(os.path.join(HERE, "anchor_head_single_v2.npz"), points=pts2.numpy(), feat=feat2.numpy(), mask=mask2.numpy(),
                        cls_preds=head2.forward_ret_dict["cls_preds"].numpy(), box_preds=head2.forward_ret_dict["box_preds"].numpy(),
                        dir_cls_preds=head2.forward_ret_dict["dir_cls_preds"].numpy(),
                        batch_cls_preds=out2["batch_cls_preds"].numpy(), batch_box_preds=out2["batch_box_preds"].numpy(), pcr=pcr, **sd2)
    print("anchor_head_single_v2: mask keeps %d of %d locations, %d boxes/sample" % (int(mask2.sum()), mask2.numel(),
                                                                                     out2["batch_box_preds"].shape[1]))
    nms_large(m)
    wide_dense(m)
    atss(m)
    proto_crop(m)
    proto_head(m)
    points_in_boxes_fixture(m)
    merge_sweeps_fixture(m)
    print("golden fixtures written to", HERE)
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print("  %-22s %8d B" % (f, os.path.getsize(os.path.join(HERE, f))))


def compiled_reference_fixture():
    """compiled_reference.npz: the compiled reference (oracle/_ref: iou3d_cpu.cpp boxes_iou_bev_cpu, roiaware_pool3d.cpp
    points_in_boxes_cpu) on exactly the inputs of the tests that compare the oracle with it -- the inputs come from those tests'
    own helpers, so the recording and the tests cannot drift apart. The tests read the recording anywhere and re-check it
    against the live reference where oracle/_ref is built. Usage:  python tests/golden/make_golden.py compiled_reference"""
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from oracle.binding import load_reference_iou, load_reference_points_in_boxes
    import test_oracle_golden
    import test_prefilter
    iou, pib = load_reference_iou(), load_reference_points_in_boxes()
    if iou is None or pib is None:
        raise SystemExit("build oracle/_ref first: make -C oracle ref")
    out = {}
    for prefix, (boxes, pts) in (("pib", test_prefilter._random_case()), ("pib_faces", test_prefilter._face_case())):
        out[prefix + ".boxes"], out[prefix + ".points"] = boxes, pts
        out[prefix + ".mask"] = np.asarray(pib(boxes, pts)).astype(np.uint8)        # 0/1: stored as bytes
    b = test_oracle_golden._live_iou_boxes()
    out["iou.boxes"], out["iou.iou"] = b, iou(b, b)
    np.savez_compressed(os.path.join(HERE, "compiled_reference.npz"), **out)
    print("compiled_reference: %s" % ", ".join("%s %s" % (k, v.shape) for k, v in out.items()))


if __name__ == "__main__":
    if sys.argv[1:] == ["compiled_reference"]:
        compiled_reference_fixture()
    else:
        main()
