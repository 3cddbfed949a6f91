"""layer_table.split_branches_at: CenterHead's branches cut for the head that runs the hm branch everywhere and the regression
branches at the peaks -- the same numbers as fuse_branches' fused layers, column for column (host only)."""
import torch

from cpd_amd import layer_table


def _branches(seed=0, c=64, outs=(2, 1, 3, 2, 3)):
    g = torch.Generator().manual_seed(seed)
    first = [(torch.randn(9, c, c, generator=g), torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)) for _ in outs]
    last = [(torch.randn(9, c, o, generator=g), torch.randn(o, generator=g)) for o in outs]
    return first, last


def test_split_reproduces_the_fused_layers():
    first, last = _branches()
    keep, c = 4, 64                                                    # the hm branch is the last one (ModelConfig.head_names)
    fw, fs, ft = zip(*first)
    lw, lb = zip(*last)
    w1, s1, t1, w2, b2, slices = layer_table.fuse_branches(fw, fs, ft, lw, lb)
    P = layer_table.split_branches_at(fw, fs, ft, lw, lb, keep)
    # first convs: rest1 | keep1 side by side are w1 / s1 / t1 (hm last), and keep1 is a whole 64-column block of them
    for fused, rest, kept in zip((w1, s1, t1), P["rest1"], P["keep1"]):
        assert torch.equal(torch.cat([rest, kept], dim=-1), fused)
        assert torch.equal(fused[..., keep * c:(keep + 1) * c], kept)
    # last convs: the fp32 image is w2's regression block, zeros included; keep2 is w2's hm block
    n_reg = sum(o for o, _ in [(w.shape[2], 0) for w in lw[:keep]])
    assert torch.equal(P["rest2"][0], w2[:, :keep * c, :n_reg]) and torch.equal(P["rest2"][1], b2[:n_reg])
    assert float(w2[:, :keep * c, n_reg:].abs().max()) == 0 and float(w2[:, keep * c:, :n_reg].abs().max()) == 0
    assert torch.equal(P["keep2"][0], w2[:, keep * c:, n_reg:]) and torch.equal(P["keep2"][1], b2[n_reg:])
    assert P["rest_slices"] == slices[:keep]
    off_diag = P["rest2"][0].clone()
    for i, (c0, n) in enumerate(P["rest_slices"]):
        off_diag[:, i * c:(i + 1) * c, c0:c0 + n] = 0
    assert float(off_diag.abs().max()) == 0                            # block-diagonal


def test_split_with_the_kept_branch_in_the_middle():
    first, last = _branches(seed=3, c=32, outs=(2, 3, 1))
    fw, fs, ft = zip(*first)
    lw, lb = zip(*last)
    P = layer_table.split_branches_at(fw, fs, ft, lw, lb, 1)
    assert torch.equal(P["keep1"][0], fw[1]) and torch.equal(P["keep2"][0], lw[1])
    assert torch.equal(P["rest1"][0], torch.cat([fw[0], fw[2]], dim=2)) and P["rest_slices"] == [(0, 2), (2, 1)]
    assert torch.equal(P["rest2"][0][:, 32:, 2:], lw[2]) and float(P["rest2"][0][:, :32, 2:].abs().max()) == 0
