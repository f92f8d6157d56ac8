"""Plain float64 references of the BatchNorm forms tests/test_batchnorm_single_gpu.py checks: eval mode behind a biased conv,
training-mode BatchNorm1d with its backward, and the R-rank combine of per-rank (sum, M2, count).  No device is needed:
tests/test_abi_and_host.py::test_bn_float64_references_match_torch compares each with torch's own float64 modules / autograd."""
import torch


def eval_reference(x, b, rm, rv, gamma, beta, eps):
    """eval-mode BatchNorm of x + b (b: the bias of the conv in front, or None)"""
    if b is not None:
        x = x + b
    return (x - rm) / torch.sqrt(rv + eps) * gamma + beta


def combine(S_r, Q_r, n_r):
    """per-rank sums S_r [R][C], M2 about the rank's own mean Q_r [R][C] and row counts n_r [R] -> (count, S, mean, M2 about
    the pooled mean)"""
    n = n_r.double()[:, None]
    cnt = float(n.sum())
    S = S_r.sum(0)
    mean = S / cnt
    M2 = (Q_r + n * (S_r / n - mean) ** 2).sum(0)
    return cnt, S, mean, M2


def bn1d_reference(x, gamma, beta, rm0, rv0, dy, eps, momentum):
    """training-mode BatchNorm1d of x [M][C] and its backward for the output gradient dy"""
    M = x.shape[0]
    S = x.sum(0)
    mean = S / M
    M2 = ((x - mean) ** 2).sum(0)
    invstd = (M2 / M + eps).rsqrt()
    xhat = (x - mean) * invstd
    sg, sgx = dy.sum(0), (dy * xhat).sum(0)
    k1 = gamma * invstd
    return dict(S=S, M2=M2, mean=mean, invstd=invstd, y=xhat * gamma + beta,
                rm=(1 - momentum) * rm0 + momentum * mean,
                rv=(1 - momentum) * rv0 + momentum * (M2 / (M - 1) if M > 1 else M2 / M),
                dx=k1 * (dy - sg / M - xhat * sgx / M), dgamma=sgx, dbeta=sg)
