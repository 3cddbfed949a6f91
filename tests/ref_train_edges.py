"""float64 numpy restatements of the operations only the train step uses: the weight gradient of the rulebook convolution, the
column reductions and row kernels of BatchNorm (+ residual + ReLU) forward and backward, and the transposed rulebooks. Plain
definitions on logical arrays -- no tiles, chunks or pitches -- for tests/test_gpu_train_edges.py to compare the HIP kernels with;
tests/test_train_edges_ref.py checks them against torch autograd in float64 on the CPU."""
import numpy as np


def wgrad_ref(x, dy, nbr, n_out):
    """dW[t] = x[nbr[t, j]]^T . dy[j] over the rows j < n_out with nbr[t, j] >= 0 (nbr None: kv = 1, dW[0] = x[:n_out]^T . dy).
    x [n_in, c_in], dy [>= n_out, c_out], nbr [kv, n_out] -> (dW [kv, c_in, c_out] float64, pairs [kv] -- the pair count per tap --,
    S [kv, c_in, c_out] = sum |x| . |dy| over the same pairs: what a summation error bound scales with)."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)[:n_out]
    kv = 1 if nbr is None else nbr.shape[0]
    assert nbr is None or nbr.shape == (kv, n_out)
    dw = np.zeros((kv, x.shape[1], dy.shape[1]))
    S = np.zeros_like(dw)
    pairs = np.zeros(kv, np.int64)
    for t in range(kv):
        if nbr is None:
            j = np.arange(n_out)
            i = j
        else:
            j = np.flatnonzero(nbr[t] >= 0)
            i = nbr[t, j]
        pairs[t] = j.size
        dw[t] = x[i].T @ dy[j]
        S[t] = np.abs(x[i]).T @ np.abs(dy[j])
    return dw, pairs, S


class bn_ref:
    """The column operations and row kernels behind training-mode BatchNorm (+ residual)(+ ReLU), in float64."""

    @staticmethod
    def col_sum(x):
        return np.asarray(x, np.float64).sum(0)

    @staticmethod
    def stats(x):
        """(sum, sum of squares) per column"""
        x = np.asarray(x, np.float64)
        return x.sum(0), (x * x).sum(0)

    @staticmethod
    def finalize(s1, s2, n, eps, momentum, gamma, beta, running_mean=None, running_var=None):
        """-> dict(mean, var (biased), invstd, scale, shift[, running_mean, running_var]); the running variance takes the unbiased
        batch variance, except at n == 1 where it keeps the biased one"""
        s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
        gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
        mean = s1 / n
        var = np.maximum(s2 / n - mean * mean, 0.0)
        invstd = 1.0 / np.sqrt(var + float(eps))
        scale = gamma * invstd
        out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=beta - mean * scale)
        if running_mean is not None:
            unbiased = var * n / (n - 1.0) if n > 1 else var
            out["running_mean"] = (1.0 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
            out["running_var"] = (1.0 - momentum) * np.asarray(running_var, np.float64) + momentum * unbiased
        return out

    @staticmethod
    def affine(x, scale=None, shift=None, res=None, relu=False):
        """y = relu(x . scale + shift + res), every term optional; ReLU as the kernels write it: v > 0 ? v : +0"""
        v = np.asarray(x, np.float64)
        if scale is not None:
            v = v * np.asarray(scale, np.float64)
        if shift is not None:
            v = v + np.asarray(shift, np.float64)
        if res is not None:
            v = v + np.asarray(res, np.float64)
        return np.where(v > 0, v, 0.0) if relu else v

    @staticmethod
    def relu_backward(g, y):
        return np.where(np.asarray(y) > 0, np.asarray(g, np.float64), 0.0)

    @staticmethod
    def backward(g, y, x, mean, invstd, gamma):
        """BatchNorm(+ residual + ReLU) backward with the mask y > 0 (y None: no ReLU) -> (dx, dgamma, dbeta, dres):
        g_m = g . mask ; dbeta = sum g_m ; dgamma = sum g_m . xhat ; dx = gamma . invstd . (g_m - dbeta/n - xhat . dgamma/n) ;
        dres = g_m"""
        g, x = np.asarray(g, np.float64), np.asarray(x, np.float64)
        mean, invstd, gamma = (np.asarray(a, np.float64) for a in (mean, invstd, gamma))
        n = x.shape[0]
        gm = g if y is None else np.where(np.asarray(y) > 0, g, 0.0)
        xhat = (x - mean) * invstd
        dbeta = gm.sum(0)
        dgamma = (gm * xhat).sum(0)
        dx = gamma * invstd * (gm - dbeta / n - xhat * dgamma / n)
        return dx, dgamma, dbeta, gm


def transpose_table(nbr, n_in):
    """nbrT[t, nbr[t, j]] = j: the input-side table of a (strided) convolution whose forward table is nbr [kv, n_out]; an input
    row feeds at most one output row per tap (asserted), the others stay -1"""
    kv = nbr.shape[0]
    out = np.full((kv, n_in), -1, np.int32)
    tt, jj = np.nonzero(nbr >= 0)
    out[tt, nbr[tt, jj]] = jj
    assert (out >= 0).sum() == tt.size, "two output rows read one input row through the same tap"
    return out


def conv2d_table(batch, h, w, kh, kw, stride, pad):
    """forward pixel table of a kh x kw convolution over (batch, h, w) maps: nbr[ky * kw + kx, (b, oy, ox)] = (b, oy . stride -
    pad + ky, ox . stride - pad + kx) as a row number, -1 outside the map -> (nbr [kh * kw, batch * ho * wo], ho, wo)"""
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    b, oy, ox = np.meshgrid(np.arange(batch), np.arange(ho), np.arange(wo), indexing="ij")
    nbr = np.full((kh * kw, batch * ho * wo), -1, np.int32)
    for ky in range(kh):
        for kx in range(kw):
            y, x = oy * stride - pad + ky, ox * stride - pad + kx
            ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
            nbr[ky * kw + kx] = np.where(ok, (b * h + y) * w + x, -1).reshape(-1)
    return nbr, ho, wo
