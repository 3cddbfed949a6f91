"""CPU: the closed form of the fused training pooling (tests/ref_pool_train.py::closed_form -- statistics and BatchNorm backward of the
linear position branch from the moments of the neighbour offsets) against float64 autograd of the restated reference sequence
(voxel_pool_modules.py:96-117). Everything agrees to 1e-10 of scale."""
import pytest
import torch

import ref_pool_train as R

TOL = 1e-10


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1.0)


@pytest.mark.parametrize("m,ns,c,empty,dup", [(257, 16, 32, 0.15, True), (65, 16, 16, 0.0, False), (33, 1, 64, 0.15, True),
                                               (17, 8, 16, 1.0, True), (1, 16, 32, 0.0, True)])
def test_closed_form_matches_autograd_of_the_restatement(m, ns, c, empty, dup):
    case = R.make_case(m, ns, c, seed=11 + m, empty=empty, dup=dup)
    t = {k: case[k].double() for k in ("fin", "xyz", "new_xyz", "w", "gamma", "beta", "grad")}
    t["beta"][3] = -50.0                                              # a channel the ReLU cuts off everywhere
    leaves = [t[k].clone().requires_grad_(True) for k in ("fin", "w", "gamma", "beta")]
    out, x, mean, var = R.restatement(leaves[0], t["xyz"], t["new_xyz"], case["idx"], leaves[1], leaves[2], leaves[3])
    out.backward(t["grad"])
    cf = R.closed_form(t["fin"], t["xyz"], t["new_xyz"], case["idx"], t["w"], t["gamma"], t["beta"], t["grad"])
    assert _rel(cf["out"], out.detach()) <= TOL
    assert _rel(cf["mean"], mean.detach()) <= TOL and _rel(cf["var"], var.detach()) <= TOL
    assert bool((cf["arg"][:, 3] == 255).all()) and float(cf["out"][:, 3].abs().max()) == 0.0
    for name, leaf in zip(("dfin", "dw", "dgamma", "dbeta"), leaves):
        assert _rel(cf[name], leaf.grad) <= TOL, name
    if empty >= 1.0:                                                  # no ball: no feature gradient, the constant relu(beta - gamma mu invstd)
        assert float(cf["dfin"].abs().max()) == 0.0
        want = torch.relu(t["beta"] - t["gamma"] * cf["mean"] * cf["invstd"])
        assert _rel(cf["out"], want[None, :].expand_as(cf["out"])) <= TOL


def test_near_tie_cells_flags_only_ties_between_different_rows():
    x = torch.tensor([[[1.0, 1.0 - 1e-6, 0.2], [1.0, 0.5, 1.0]]]).double()        # (M = 1, C = 2, ns = 3)
    idx = torch.tensor([[4, 7, 4]], dtype=torch.int32)
    tie = R.near_tie_cells(x, idx)
    assert tie.tolist() == [[True, False]]                           # channel 1's equal candidates are the same row (a pre-filled slot)
