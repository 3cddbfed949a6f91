"""CPU: plan_target_draws, the host half of the device proposal-target layer (cpd_amd.roi_head_train), against
ProposalTargetLayer.subsample_rois on CPU overlap vectors under equal seeds: the pools the classify kernel would emit (nonzero()
order) indexed by the planner's picks are the torch path's selection index for index, and both paths leave numpy's and torch's
generators in the same state (the planner consumed exactly as many numbers)."""
import numpy as np
import pytest
import torch

SCALAR = dict(ROI_PER_IMAGE=16, FG_RATIO=0.5, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
              HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
LISTS = dict(ROI_PER_IMAGE=16, FG_RATIO=0.5, CLS_SCORE_TYPE="roi_iou_x", CLS_FG_THRESH=[0.75, 0.6, 0.65], CLS_BG_THRESH=[0.25, 0.15, 0.2],
             CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=[0.55, 0.4, 0.45], HARD_SAMPLING_THRESH=[0.3, 0.2, 0.25],
             HARD_SAMPLING_RATIO=[0.5, 0.25, 0.34])


def _pools(overlaps, cfg, gts):
    """the three pools as the classify kernel defines them, in nonzero() order"""
    lo = cfg["CLS_BG_THRESH_LO"]
    easy = overlaps < lo
    if gts is None:
        fg = overlaps >= min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])
        hard = (overlaps < cfg["REG_FG_THRESH"]) & (overlaps >= lo)
    else:
        fg, hard = torch.zeros_like(easy), torch.zeros_like(easy)
        for c, (r, k) in enumerate(zip(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])):
            own = gts[:, -1] == c + 1
            fg |= own & (overlaps >= min(r, k))
            hard |= own & (overlaps < r) & (overlaps >= lo)
    return [m.nonzero().view(-1) for m in (fg, hard, easy)]


def _frame(kind, n, gen):
    """overlaps of one frame whose pools have the wanted make-up (values well away from every threshold)"""
    fg, hard, easy = 0.8 + 0.15 * torch.rand(n, generator=gen), 0.12 + 0.2 * torch.rand(n, generator=gen), 0.08 * torch.rand(n, generator=gen)
    pick = torch.randint(0, 3, (n,), generator=gen)
    allowed = {"fg_bg": (0, 1, 2), "fg_only": (0,), "hard_only": (1,), "easy_only": (2,), "hard_easy": (1, 2), "few_fg": (1, 2), "fg_hard": (0, 1)}[kind]
    pick = torch.tensor(allowed)[pick % len(allowed)]
    ov = torch.where(pick == 0, fg, torch.where(pick == 1, hard, easy))
    if kind == "few_fg":                                              # fewer foreground RoIs than the quota of 8
        ov[:3] = fg[:3]
    return ov


CASES = [("fg_bg",), ("fg_only",), ("hard_only",), ("easy_only",), ("hard_easy",), ("few_fg",), ("fg_bg", "fg_only", "hard_easy"),
         ("few_fg", "easy_only", "fg_hard")]


@pytest.mark.parametrize("per_class", [False, True])
@pytest.mark.parametrize("hard_ratio", [0.8, 0.01])                   # 0.01: int(num * hard_ratio) = 0, a zero-size randint call
@pytest.mark.parametrize("case", range(len(CASES)))
def test_planner_reproduces_subsample_rois(case, hard_ratio, per_class):
    from cpd_amd.roi_head_train import ProposalTargetLayer, plan_target_draws
    cfg = dict(LISTS if per_class else SCALAR, HARD_BG_RATIO=hard_ratio)
    layer = ProposalTargetLayer(cfg)
    gen = torch.Generator().manual_seed(100 + case)
    frames = []
    for kind in CASES[case]:
        ov = _frame(kind, 37, gen)
        gts = torch.cat([torch.zeros(37, 7), torch.randint(1, 4, (37, 1), generator=gen).float()], 1) if per_class else None
        frames.append((ov, gts))
    seed = 7 + case
    np.random.seed(seed)
    torch.manual_seed(seed)
    want = [layer.subsample_rois(ov, gts=gts) for ov, gts in frames]
    tail_want = (np.random.rand(), float(torch.rand(1)))
    np.random.seed(seed)
    torch.manual_seed(seed)
    lists = [_pools(ov, cfg, gts) for ov, gts in frames]
    picks, offsets = plan_target_draws([[len(p) for p in ls] for ls in lists], cfg)
    tail_got = (np.random.rand(), float(torch.rand(1)))
    assert picks.shape == (len(frames), 16, 2) and picks.dtype == np.int32 and offsets is None
    for ls, pk, sel in zip(lists, picks, want):
        got = torch.stack([ls[int(pool)][int(pos)] for pool, pos in pk])
        assert torch.equal(got, sel)
    assert tail_got == tail_want
    if CASES[case] == ("few_fg",):
        assert int((picks[0, :, 0] == 0).sum()) == 3                  # the quota is 8
    if CASES[case] == ("fg_only",):
        assert bool((picks[0, :, 0] == 0).all())


@pytest.mark.parametrize("hard", [False, True])
def test_planner_makes_the_hard_sampling_draws_after_all_frames(hard):
    """ENABLE_HARD_SAMPLING: one np.random.randint(0, int(1 / ratio)) per class after the sampling's own draws (forward, l.66-72)."""
    from cpd_amd.roi_head_train import ProposalTargetLayer, plan_target_draws
    cfg = dict(LISTS, ENABLE_HARD_SAMPLING=hard)
    layer = ProposalTargetLayer(cfg)
    gen = torch.Generator().manual_seed(3)
    frames = []
    for kind in ("fg_bg", "hard_easy", "fg_bg"):
        frames.append((_frame(kind, 50, gen), torch.cat([torch.zeros(50, 7), torch.randint(1, 4, (50, 1), generator=gen).float()], 1)))
    np.random.seed(11)
    torch.manual_seed(11)
    for ov, gts in frames:
        layer.subsample_rois(ov, gts=gts)
    want = [np.random.randint(0, int(1 / r)) for r in cfg["HARD_SAMPLING_RATIO"]] if hard else None
    tail_want = (np.random.rand(), float(torch.rand(1)))
    np.random.seed(11)
    torch.manual_seed(11)
    _, offsets = plan_target_draws([[len(p) for p in _pools(ov, cfg, gts)] for ov, gts in frames], cfg)
    assert offsets == want
    assert (np.random.rand(), float(torch.rand(1))) == tail_want


def test_planner_raises_at_the_frame_with_neither_pool():
    from cpd_amd.roi_head_train import plan_target_draws
    np.random.seed(5)
    torch.manual_seed(5)
    np.random.permutation(4)                                          # frame 0's draws are made before frame 1 raises: 4 fg of a quota of 8,
    torch.randint(low=0, high=3, size=(12,))                          # 12 hard negatives; frame 2 does not get its turn
    tail_want = (np.random.rand(), float(torch.rand(1)))
    np.random.seed(5)
    torch.manual_seed(5)
    with pytest.raises(NotImplementedError):
        plan_target_draws([[4, 3, 0], [0, 0, 0], [2, 2, 2]], SCALAR)
    assert (np.random.rand(), float(torch.rand(1))) == tail_want


def test_switch_is_off_by_default_and_set_fused_targets_counts_layers():
    from cpd_amd.roi_head_train import ProposalTargetLayer, set_fused_targets
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), ProposalTargetLayer(SCALAR), torch.nn.Sequential(ProposalTargetLayer(LISTS)))
    layers = [m for m in model.modules() if isinstance(m, ProposalTargetLayer)]
    assert [m.fused for m in layers] == [False, False]
    assert set_fused_targets(model) == 2 and all(m.fused for m in layers)
    assert set_fused_targets(model, on=False) == 2 and not any(m.fused for m in layers)
    # host tensors never take the device path, switch or not
    layers[0].fused = True
    bd = {"batch_size": 1, "rois": torch.zeros(1, 4, 7), "roi_scores": torch.zeros(1, 4), "roi_labels": torch.ones(1, 4, dtype=torch.long),
          "gt_boxes": torch.zeros(1, 2, 8)}
    assert not layers[0].fused_ok(bd)
