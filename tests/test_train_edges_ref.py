"""tests/ref_train_edges.py against torch autograd in float64 on the CPU, to 1e-12 relative: the restatements the GPU edge suite
(tests/test_gpu_train_edges.py) trusts are themselves checked against an independent derivation of the same gradients."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_train_edges as R

RTOL = 1e-12


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    assert err <= RTOL, (what, err)


def gather_matmul(x, w_kio, nbr):
    """sum_t x[nbr[t]] @ W[t], masked -- the autograd form of the rulebook convolution (as tests/test_gpu_train_ops.py writes it)"""
    out = 0
    for t in range(nbr.shape[0]):
        idx = torch.from_numpy(nbr[t].astype(np.int64))
        g = x[idx.clamp_min(0)] * (idx >= 0).to(x.dtype)[:, None]
        out = out + g @ w_kio[t]
    return out


@pytest.mark.parametrize("kv,n_in,n_out,cin,cout", [(27, 23, 41, 5, 7), (9, 50, 17, 8, 3), (1, 9, 9, 4, 6)])
def test_wgrad_ref_matches_autograd(kv, n_in, n_out, cin, cout):
    rng = np.random.default_rng(kv + n_out)
    nbr = rng.integers(0, n_in, size=(kv, n_out)).astype(np.int32)
    nbr[rng.random((kv, n_out)) < 0.5] = -1
    if kv > 1:
        nbr[kv // 2] = -1                         # a tap nobody has
    x, dy = rng.normal(size=(n_in, cin)), rng.normal(size=(n_out + 3, cout))
    w = rng.normal(size=(kv, cin, cout))
    xt, wt = torch.tensor(x), torch.tensor(w, requires_grad=True)
    gather_matmul(xt, wt, nbr).backward(torch.tensor(dy[:n_out]))
    dw, pairs, S = R.wgrad_ref(x, dy, nbr, n_out)
    close(dw, wt.grad.numpy(), "dW")
    assert pairs.tolist() == (nbr >= 0).sum(1).tolist()
    # S is the same sum over the absolute values: it bounds |dW| and equals it for non-negative operands
    assert (np.abs(dw) <= S * (1 + 1e-12)).all()
    dw_abs, _, S_abs = R.wgrad_ref(np.abs(x), np.abs(dy), nbr, n_out)
    close(S, dw_abs, "S")
    close(S_abs, dw_abs, "S of non-negative operands")
    if kv > 1:
        assert not dw[kv // 2].any() and not S[kv // 2].any() and pairs[kv // 2] == 0


def test_wgrad_ref_without_a_table():
    rng = np.random.default_rng(2)
    x, dy = rng.normal(size=(12, 5)), rng.normal(size=(9, 4))
    dw, pairs, S = R.wgrad_ref(x, dy, None, 7)
    close(dw[0], x[:7].T @ dy[:7], "dW, no table")
    close(S[0], np.abs(x[:7]).T @ np.abs(dy[:7]), "S, no table")
    assert dw.shape == (1, 5, 4) and pairs.tolist() == [7]


@pytest.mark.parametrize("n,c", [(1, 3), (2, 5), (65, 4), (300, 7)])
def test_bn_ref_matches_autograd(n, c):
    rng = np.random.default_rng(n * 7 + c)
    eps, momentum = 1e-3, 0.1
    x = rng.normal(size=(n, c)) * rng.uniform(0.5, 2, c) + rng.normal(size=c)
    res, g = rng.normal(size=(n, c)), rng.normal(size=(n, c))
    gamma, beta = rng.uniform(0.5, 1.5, c), rng.normal(size=c)
    rm, rv = rng.normal(size=c), rng.uniform(0.5, 2, c)
    xt, rt = torch.tensor(x, requires_grad=True), torch.tensor(res, requires_grad=True)
    gt, bt = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    if n > 1:                                    # (torch refuses a training batch of one value per channel)
        rmt, rvt = torch.tensor(rm), torch.tensor(rv)
        yt = F.relu(F.batch_norm(xt, rmt, rvt, gt, bt, training=True, momentum=momentum, eps=eps) + rt)
    s1, s2 = R.bn_ref.stats(x)
    close(s1, x.sum(0), "sum")
    close(R.bn_ref.col_sum(x), x.sum(0), "col_sum")
    close(s2, (x * x).sum(0), "sumsq")
    f = R.bn_ref.finalize(s1, s2, n, eps, momentum, gamma, beta, rm, rv)
    y = R.bn_ref.affine(x, f["scale"], f["shift"], res, True)
    dx, dgamma, dbeta, dres = R.bn_ref.backward(g, y, x, f["mean"], f["invstd"], gamma)
    if n == 1:
        # one row: the mean is the row, the variance 0 (biased, and kept biased for the running update), dx = 0
        close(f["mean"], x[0], "mean, n = 1")
        assert not f["var"].any()
        close(f["invstd"], np.full(c, 1 / np.sqrt(eps)), "invstd, n = 1")
        close(f["running_var"], (1 - momentum) * rv, "running_var, n = 1")
        close(y, np.maximum(beta + res, 0), "y, n = 1")
        assert np.abs(dx).max() <= 1e-9
        return
    yt.backward(torch.tensor(g))
    # (sumsq / n - mean^2 loses digits to the subtraction where torch's two-pass variance does not: compared at the
    # conditioning of these columns, |mean| <= 3 sigma, a few units of 1e-16 become a few of 1e-15)
    np.testing.assert_allclose(f["var"], x.var(0), rtol=1e-12, atol=0)
    close(f["mean"], x.mean(0), "mean")
    close(f["running_mean"], rmt.numpy(), "running_mean")
    close(f["running_var"], rvt.numpy(), "running_var")
    close(y, yt.detach().numpy(), "y")
    close(dres, rt.grad.numpy(), "dres")
    close(dbeta, bt.grad.numpy(), "dbeta")
    close(dgamma, gt.grad.numpy(), "dgamma")
    close(dx, xt.grad.numpy(), "dx")
    close(R.bn_ref.relu_backward(g, y), g * (y > 0), "relu_backward")


def test_bn_ref_mask_is_strict_and_signed_zero_safe():
    y = np.array([[0.0, -0.0, -1.0, 2.0]])
    g = np.array([[3.0, 5.0, 7.0, 9.0]])
    assert R.bn_ref.relu_backward(g, y).tolist() == [[0.0, 0.0, 0.0, 9.0]]
    dx, dgamma, dbeta, dres = R.bn_ref.backward(g, y, np.zeros((1, 4)), np.zeros(4), np.ones(4), np.ones(4))
    assert dres.tolist() == [[0.0, 0.0, 0.0, 9.0]] and dbeta.tolist() == [0.0, 0.0, 0.0, 9.0]
    v = R.bn_ref.affine(np.array([[-2.0, 0.0, 1.0]]), relu=True)
    assert v.tolist() == [[0.0, 0.0, 1.0]] and not np.signbit(v).any()


@pytest.mark.parametrize("h,w,k,stride,pad", [(1, 1, 3, 1, 1), (5, 7, 3, 2, 1), (6, 6, 2, 2, 0), (7, 5, 3, 2, 0), (4, 4, 1, 1, 0)])
@pytest.mark.parametrize("batch", [1, 3])
def test_conv2d_tables_match_torch_conv2d(batch, h, w, k, stride, pad):
    """the forward pixel table reproduces F.conv2d, and the gather through its transposed table (weights transposed, taps as they
    are) reproduces F.conv2d's input gradient"""
    rng = np.random.default_rng(h * 10 + w)
    cin, cout = 3, 4
    nbr, ho, wo = R.conv2d_table(batch, h, w, k, k, stride, pad)
    assert nbr.shape == (k * k, batch * ho * wo) and nbr.min() >= -1 and nbr.max() < batch * h * w
    x, wt = rng.normal(size=(batch, cin, h, w)), rng.normal(size=(cout, cin, k, k))
    xt, wtt = torch.tensor(x, requires_grad=True), torch.tensor(wt)
    y = F.conv2d(xt, wtt, None, stride, pad)
    assert tuple(y.shape[2:]) == (ho, wo)
    dy = rng.normal(size=tuple(y.shape))
    y.backward(torch.tensor(dy))
    rows = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1).reshape(-1, a.shape[1]))
    w_kio = wtt.permute(2, 3, 1, 0).reshape(k * k, cin, cout)
    close(gather_matmul(torch.tensor(rows(x)), w_kio, nbr).numpy(), rows(y.detach().numpy()), "conv2d forward")
    nbr_t = R.transpose_table(nbr, batch * h * w)
    assert nbr_t.shape == (k * k, batch * h * w)
    dx = gather_matmul(torch.tensor(rows(dy)), w_kio.transpose(1, 2), nbr_t).numpy()
    close(dx, rows(xt.grad.numpy()), "conv2d input gradient")
    # and the definition, entry by entry
    for t, j in zip(*np.nonzero(nbr >= 0)):
        assert nbr_t[t, nbr[t, j]] == j
    assert (nbr_t >= 0).sum() == (nbr >= 0).sum()


def test_transpose_table_refuses_a_table_that_is_not_a_convolution():
    with pytest.raises(AssertionError):
        R.transpose_table(np.array([[0, 0]], np.int32), 2)
