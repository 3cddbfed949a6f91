"""cpd_anchor_assign_batch (AxisAlignedTargetAssigner.fused, anchor_head.assign_targets_batch): the whole batch's anchor targets in
at most three launches. Against the host loop over cpd_anchor_assign bit for bit -- the kernels are deterministic and run the same
device functions in the same order -- and against tests/ref_anchor_batch.py (the CPU oracle per frame and set; its own checks are in
test_anchor_batch_ref.py) with the bounds of test_anchor_head.py: labels, IoUs and weights exact, targets within 2e-6."""
import numpy as np
import pytest

import ref_anchor_batch as rab

pytestmark = pytest.mark.gpu
KEYS = ("box_cls_labels", "box_reg_targets", "reg_weights", "gt_ious")


def _assigner(ah, cfgs, fused, norm=False, classes=rab.CLASSES):
    a = ah.AxisAlignedTargetAssigner(cfgs, classes, norm_by_num_examples=norm)
    assert a.fused is False                                          # the switch is off by default
    a.fused = fused
    return a


def _both(ah, cfgs, anchors, gt, norm=False):
    loop = _assigner(ah, cfgs, False, norm).assign_targets(anchors, gt)
    fused = _assigner(ah, cfgs, True, norm).assign_targets(anchors, gt)
    assert tuple(fused) == tuple(loop) == KEYS
    for k in KEYS:
        assert fused[k].dtype == loop[k].dtype and fused[k].shape == loop[k].shape
        np.testing.assert_array_equal(fused[k].cpu().numpy(), loop[k].cpu().numpy(), err_msg=k)
    return {k: v.cpu().numpy() for k, v in loop.items()}


@pytest.fixture(scope="module")
def small(hip):
    import torch
    from cpd_amd import anchor_head as ah
    cfgs = rab.small_cfgs()
    anchors, _ = ah.AnchorGenerator(rab.SMALL_RANGE, cfgs).generate_anchors([rab.SMALL_GRID] * 3)
    assert all(tuple(a.shape) == (1, 9, 11, 1, 2, 7) for a in anchors)
    return ah, cfgs, anchors, torch.from_numpy(rab.small_gt()).cuda()


@pytest.fixture(scope="module")
def small_ref(oracle, small):
    _, cfgs, anchors, gt = small
    sets = [a.cpu().numpy() for a in anchors]
    return {norm: rab.ref_anchor_batch(oracle, sets, gt.cpu().numpy(), rab.CLASSES, rab.CLASSES, rab.thresholds(cfgs), norm)
            for norm in (False, True)}


@pytest.mark.parametrize("norm", [False, True])
def test_small_case_equals_the_loop_and_the_oracle(small, small_ref, norm):
    ah, cfgs, anchors, gt = small
    _both(ah, cfgs, anchors, gt, norm)
    asg = _assigner(ah, cfgs, True, norm)
    got = ah.assign_targets_batch(anchors, gt, asg.class_names, asg.anchor_class_names, asg.matched, asg.unmatched, norm)
    ref = small_ref[norm]
    np.testing.assert_array_equal(got["box_cls_labels"].cpu().numpy(), ref["labels"])
    np.testing.assert_array_equal(got["gt_ious"].cpu().numpy(), ref["gt_ious"])
    np.testing.assert_array_equal(got["reg_weights"].cpu().numpy(), ref["reg_weights"])
    np.testing.assert_allclose(got["box_reg_targets"].cpu().numpy(), ref["reg_targets"], rtol=0, atol=2e-6)
    np.testing.assert_array_equal(got["gt_max_iou"].cpu().numpy(), ref["gt_max_iou"])
    np.testing.assert_array_equal(got["n_examples"].cpu().numpy(), ref["n_examples"])
    assert int((ref["labels"] > 0).sum()) >= 10 and int((ref["labels"] == -1).sum()) >= 1


def test_masked_anchors_cross_a_block_with_outer_k_and_inner_two(small):
    """The heads' masked form (1, K, 1, 2, 7): K = 129 of the 135 locations of a 15 x 9 grid, 258 anchors per set."""
    import torch
    ah, cfgs, _, gt = small
    root, _ = ah.AnchorGenerator([0.0, -10.0, -2.0, 28.0, 10.0, 4.0], cfgs).generate_anchors([[15, 9]] * 3)
    mask = torch.ones(9, 15, dtype=torch.bool)
    for h, w in ((0, 14), (1, 13), (4, 0), (4, 12), (7, 11), (8, 14)):
        mask[h, w] = False
    mask = mask.cuda()
    anchors = [a[:, mask, ...] for a in root]
    assert all(tuple(a.shape) == (1, 129, 1, 2, 7) for a in anchors)
    loop = _both(ah, cfgs, anchors, gt)
    for c in (1, 2, 3):                                              # every class has boxes somewhere in the batch
        assert int((loop["box_cls_labels"] == c).sum()) >= 1
    _both(ah, cfgs, anchors, gt, norm=True)


def test_more_rows_than_threads_and_an_empty_frame(small):
    """m = 300 > 256: the staging loop and the compaction take several rows per thread."""
    import torch
    ah, cfgs, anchors, _ = small
    rng = np.random.default_rng(11)
    gt = np.zeros((2, 300, 8), np.float32)
    gt[0] = np.concatenate([rng.uniform(0, 20, (300, 1)), rng.uniform(-10, 10, (300, 1)), rng.uniform(-1, 1, (300, 1)),
                            np.array([4.7, 2.1, 1.7]) * rng.uniform(0.8, 1.2, (300, 3)), rng.uniform(-3.1, 3.1, (300, 1)),
                            np.ones((300, 1))], 1)
    loop = _both(ah, cfgs, anchors, torch.from_numpy(gt).cuda())
    assert int((loop["box_cls_labels"][0] == 1).sum()) >= 50 and int((loop["box_cls_labels"][1] != 0).sum()) == 0
    _both(ah, cfgs, anchors, torch.from_numpy(gt).cuda(), norm=True)


def test_fused_assigner_meets_the_reference_golden(golden, hip):
    import torch
    from cpd_amd import anchor_head as ah
    g = golden("anchor_head")
    cfgs = [dict(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0], matched_threshold=mt,
                 unmatched_threshold=ut)
            for n, s, mt, ut in (("Vehicle", [4.7, 2.1, 1.7], 0.55, 0.4), ("Pedestrian", [0.91, 0.86, 1.73], 0.5, 0.35),
                                 ("Cyclist", [1.78, 0.84, 1.78], 0.5, 0.35))]
    anchors = [torch.from_numpy(a).cuda() for a in g["anchors_per_class"]]
    tgt = _assigner(ah, cfgs, True).assign_targets(anchors, torch.from_numpy(g["gt"]).cuda())
    np.testing.assert_array_equal(tgt["box_cls_labels"].cpu().numpy(), g["labels"])
    np.testing.assert_array_equal(tgt["gt_ious"].cpu().numpy(), g["gt_ious"])
    np.testing.assert_array_equal(tgt["reg_weights"].cpu().numpy(), g["reg_weights"])
    np.testing.assert_allclose(tgt["box_reg_targets"].cpu().numpy(), g["reg_targets"], rtol=0, atol=2e-6)


def test_heads_train_forward_and_loss_do_not_change_with_the_switch(golden, hip):
    """AnchorHeadSingleV2 in .train() (input as test_v2_head_and_proto_head_train_one_step_end_to_end builds it):
    set_fused_anchor_targets flips the head's one assigner; targets, gt_ious and the training loss stay bit for bit."""
    import torch
    from cpd_amd import anchor_head as ah
    g2, gp = golden("anchor_head_single_v2"), golden("proto_head")
    cfgs = [dict(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0], align_center=False,
                 feature_map_stride=8, matched_threshold=0.5, unmatched_threshold=0.35)
            for n, s in (("Vehicle", [4.7, 2.1, 1.7]), ("Pedestrian", [0.91, 0.86, 1.73]), ("Cyclist", [1.78, 0.84, 1.78]))]
    mcfg = dict(ANCHOR_GENERATOR_CONFIG=cfgs, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
                TARGET_ASSIGNER_CONFIG=dict(NAME="AxisAlignedTargetAssigner", NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False),
                LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0] * 7)))
    head = ah.AnchorHeadSingleV2(mcfg, 32, 3, rab.CLASSES, np.array([416, 416, 40]), g2["pcr"].tolist(), conv_math="f32")
    head.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g2.items() if k.startswith("v2.")})
    head = head.cuda().train()

    def step():
        dd = {"points": torch.from_numpy(g2["points"]).cuda(), "st_features_2d": torch.from_numpy(g2["feat"]).cuda(), "batch_size": 2,
              "gt_boxes": torch.from_numpy(gp["gt"]).cuda()}
        dd = head(dd)
        f = head.forward_ret_dict
        loss, tb = head.get_training_loss()
        return {"labels": f["box_cls_labels"], "targets": f["box_reg_targets"], "weights": f["reg_weights"],
                "gt_ious": dd["gt_ious"], "ret_ious": f["gt_ious"], "loss": loss.detach()}, tb

    assert head.target_assigner.fused is False
    off, tb_off = step()
    assert ah.set_fused_anchor_targets(head) == 1 and head.target_assigner.fused is True
    on, tb_on = step()
    assert int((off["labels"] > 0).sum()) > 0
    for k in off:
        assert on[k].dtype == off[k].dtype and on[k].shape == off[k].shape
        np.testing.assert_array_equal(on[k].cpu().numpy(), off[k].cpu().numpy(), err_msg=k)
    assert tb_on == tb_off
    assert ah.set_fused_anchor_targets(head, on=False) == 1 and head.target_assigner.fused is False
    eval_only = ah.AnchorHeadSingle({k: v for k, v in mcfg.items() if k != "TARGET_ASSIGNER_CONFIG"}, 24, 3, rab.CLASSES,
                                    np.array([416, 416, 40]), g2["pcr"].tolist())
    assert ah.set_fused_anchor_targets(torch.nn.ModuleList([head, eval_only])) == 1   # no assigner config: nothing to flip


def test_bad_arguments_are_refused_before_anything_is_launched(small):
    import torch
    from cpd_amd import _lib
    ah, cfgs, anchors, gt = small
    lib = _lib.lib()
    flat = torch.cat([a.reshape(-1, 7) for a in anchors]).contiguous()
    n = flat.shape[0]
    out = [torch.full((2, n), 77, dtype=torch.int32, device="cuda"), torch.full((2, n, 7), 77.0, device="cuda"),
           torch.full((2, n), 77.0, device="cuda"), torch.full((2, n), 77.0, device="cuda"),
           torch.full((2, 2049), 77.0, device="cuda"), torch.full((2, 9), 77, dtype=torch.int32, device="cuda")]
    big = torch.zeros((2, 2049, 8), device="cuda")

    def call(n_sets, set_n, set_inner, batch, m):
        cls = list(range(1, n_sets + 1))
        rc = lib.cpd_anchor_assign_batch(_lib.ptr(flat), n_sets, _lib.iarr(set_n), _lib.iarr(set_inner), _lib.iarr(cls),
                                         _lib.farr([0.55] * n_sets), _lib.farr([0.4] * n_sets), max(n_sets, 3), _lib.ptr(big), batch, m, 8,
                                         0, *[_lib.ptr(t) for t in out], _lib.stream())
        torch.cuda.synchronize()
        return rc

    assert call(3, [198] * 3, [22] * 3, 2, 2049) == -1               # m > 2048
    assert call(9, [66] * 9, [22] * 9, 2, 8) == -1                   # more than 8 sets
    assert call(3, [198] * 3, [22, 22, 11], 2, 8) == -1              # outer 9, 9, 18
    for t in out:
        assert bool((t == 77).all())                                 # nothing was written
    assert call(3, [198] * 3, [22] * 3, 0, 8) == 0                   # an empty batch is no error
    for t in out:
        assert bool((t == 77).all())
    assert call(3, [198] * 3, [22] * 3, 2, 8) == 0                   # the same call with a batch: all-zero frames are background
    assert bool((out[0] == 0).all()) and bool((out[4].view(-1)[:2 * 8] == 0).all()) and bool((out[5].view(-1)[:2 * 3] == 198).all())
