"""float64 torch restatement of one scale of NeighborVoxelSAModuleMSG.forward in training (voxel_pool_modules.py:96-117: grouping,
empty-ball masks, mlps_pos = Conv2d(3, C, bias=False) + BatchNorm2d on batch statistics, add, ReLU, max-pool over the samples), and the
closed form the fused kernels (cpd_voxel_pool_moments / cpd_voxel_pool_max_train / cpd_voxel_pool_max_train_grad) evaluate. CPU only.

idx_raw is the query kernel's output: global rows, idx_raw[m, 0] < 0 for an empty ball."""
import numpy as np
import torch
import torch.nn.functional as F


def make_case(m, ns, c, n=50, seed=0, empty=0.15, frames=2, dup=True):
    """Seeded Gaussian inputs of one scale: n feature rows over `frames` frames (a grid point draws its neighbours from its own frame's
    rows), a share `empty` of empty balls, random duplicate pre-fill (the slots behind a random count repeat slot 0)."""
    g = torch.Generator().manual_seed(seed)
    fin = torch.randn(n, c, generator=g)
    xyz = torch.randn(n, 3, generator=g)
    new_xyz = torch.randn(m, 3, generator=g)
    per, per_m = n // frames, -(-m // frames)
    idx = torch.empty((m, ns), dtype=torch.int64)
    for i in range(m):
        f = min(i // per_m, frames - 1)
        lo, hi = f * per, (n if f == frames - 1 else (f + 1) * per)
        idx[i] = lo + torch.randperm(hi - lo, generator=g)[torch.arange(ns) % (hi - lo)]
        if dup:
            cnt = int(torch.randint(1, ns + 1, (1,), generator=g))
            idx[i, cnt:] = idx[i, 0]
    if empty >= 1.0:
        is_empty = torch.ones(m, dtype=torch.bool)
    elif empty <= 0.0:
        is_empty = torch.zeros(m, dtype=torch.bool)
    else:
        is_empty = torch.rand(m, generator=g) < empty
    idx[is_empty] = 0
    idx[is_empty, 0] = -1
    w = torch.randn(c, 3, generator=g) * (2.0 / 3.0) ** 0.5            # kaiming_normal_ of Conv2d(3, c, 1)
    gamma = 1.0 + 0.2 * torch.randn(c, generator=g)
    beta = 0.3 * torch.randn(c, generator=g)
    grad = torch.randn(m, c, generator=g)
    rm, rv = 0.1 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    return dict(fin=fin, xyz=xyz, new_xyz=new_xyz, idx=idx.int(), w=w, gamma=gamma, beta=beta, grad=grad, running_mean=rm, running_var=rv,
                frames=frames, per=per, per_m=per_m)


def restatement(fin, xyz, new_xyz, idx_raw, w, gamma, beta, eps=1e-5):
    """The reference sequence on float64 tensors (autograd flows into fin, w, gamma, beta). Returns (out [M, C], x [M, C, ns] = the
    activations the max-pool sees, mean [C], biased var [C])."""
    idx = idx_raw.long()
    empty = idx[:, 0] < 0
    idx = torch.where(empty[:, None], torch.zeros_like(idx), idx)
    keep = (~empty).to(fin.dtype)[:, None, None]
    gf = fin[idx].permute(0, 2, 1) * keep                                              # (M, C, ns); l.96-99
    gx = (xyz[idx].permute(0, 2, 1) - new_xyz.unsqueeze(-1)) * keep                    # (M, 3, ns); l.104-105
    pos = F.conv2d(gx.permute(1, 0, 2).unsqueeze(0), w[:, :, None, None])              # (1, C, M, ns); l.109
    mean = pos.mean(dim=(0, 2, 3))
    var = pos.var(dim=(0, 2, 3), unbiased=False)
    pos = (pos - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps) * gamma[None, :, None, None] + beta[None, :, None, None]
    x = torch.relu(gf.permute(1, 0, 2).unsqueeze(0) + pos)                             # l.110-111
    out = F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)                      # l.114-116
    return out.squeeze(0).permute(1, 0), x.squeeze(0).permute(1, 0, 2), mean, var


def running_update(running_mean, running_var, mean, var, n, momentum=0.1):
    """torch's BatchNorm rule: momentum and the unbiased variance"""
    return (1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * var * n / (n - 1)


def closed_form(fin, xyz, new_xyz, idx_raw, w, gamma, beta, grad, eps=1e-5):
    """What the fused kernels compute, in float64 without autograd: statistics from the moments S1, S2 of p, forward with the first-
    maximum argmax (255 where the ReLU cuts the maximum off), backward from the sums over the argmax slots."""
    fin, xyz, new_xyz, w, gamma, beta, grad = [t.detach().double() for t in (fin, xyz, new_xyz, w, gamma, beta, grad)]
    idx = idx_raw.long()
    m, ns = idx.shape
    c = w.shape[0]
    empty = idx[:, 0] < 0
    idx = torch.where(empty[:, None], torch.zeros_like(idx), idx)
    keep = (~empty).double()
    p = (xyz[idx] - new_xyz[:, None, :]) * keep[:, None, None]                          # (M, ns, 3)
    n = float(m * ns)
    s1 = p.sum(dim=(0, 1))
    s2 = torch.einsum("msi,msj->ij", p, p)
    mean = w @ s1 / n
    var = torch.einsum("ci,ij,cj->c", w, s2 / n - torch.outer(s1, s1) / n ** 2, w)
    invstd = 1.0 / torch.sqrt(var + eps)
    zhat = (torch.einsum("msi,ci->msc", p, w) - mean) * invstd                          # (M, ns, C)
    x = torch.relu(fin[idx] * keep[:, None, None] + gamma * zhat + beta)
    out, arg = x.max(dim=1)                                                             # (torch returns the first maximum on CPU)
    first = (x == out[:, None, :]).double().argmax(dim=1)
    assert torch.equal(first, arg)
    live = out > 0
    arg = torch.where(live, arg, torch.full_like(arg, 255))
    G = torch.where(live, grad, torch.zeros_like(grad))                                 # (M, C)
    a = torch.where(live, arg, torch.zeros_like(arg))
    rows = torch.gather(idx, 1, a)                                                      # (M, C): the feature row of the argmax
    p_star = torch.gather(p, 1, a[:, :, None].expand(m, c, 3))                          # (M, C, 3)
    z_star = torch.gather(zhat, 1, a[:, None, :]).squeeze(1)                            # (M, C)
    dbeta = G.sum(0)
    dgamma = (G * z_star).sum(0)
    dfin = torch.zeros_like(fin)
    ch = torch.arange(c)[None, :].expand(m, c)
    dfin.index_put_((rows.reshape(-1), ch.reshape(-1)), (G * keep[:, None]).reshape(-1), accumulate=True)
    gp = torch.einsum("mc,mci->ci", G, p_star)
    dw = (gamma * invstd)[:, None] * (gp - dbeta[:, None] / n * s1[None, :]
                                      - (dgamma / n * invstd)[:, None] * (w @ s2 - mean[:, None] * s1[None, :]))
    return dict(out=out, arg=arg, mean=mean, var=var, invstd=invstd, dfin=dfin, dw=dw, dgamma=dgamma, dbeta=dbeta)


def near_tie_cells(x, idx_raw, tol=1e-5):
    """(M, C) bool: cells whose best and second-best candidates (float64 activations x [M, C, ns]) come from DIFFERENT feature rows and
    lie within `tol` of each other -- fp32 rounding may route their gradient to the other row."""
    idx = idx_raw.long()
    idx = torch.where(idx[:, :1] < 0, torch.zeros_like(idx), idx)
    best, arg = x.max(dim=2)
    row = torch.gather(idx, 1, arg)                                                     # (M, C)
    other = idx[:, None, :] != row[:, :, None]                                          # (M, C, ns)
    second = torch.where(other, x, torch.full_like(x, -np.inf)).max(dim=2)[0]
    return (best - second) <= tol
