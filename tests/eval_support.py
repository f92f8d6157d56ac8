"""Test data the clip-feature evaluation suites (k-NN, ranking) share."""
import torch

CACHE = {}


def grid_rows(seed, R, n):
    """multiples of 1/4 in [-2, 2], fp32, on the host"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (R, n), generator=gen).float() / 4


def chunks_of(n, m, descending=False):
    c = [(s, min(m, n - s)) for s in range(0, n, m)]
    return c[::-1] if descending else c


def unit_gauss(gen, n, D):
    x = torch.randn((n, D), generator=gen, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()


def knn_eval_case(gpu):
    """130 test and 1000 train features of 512 dimensions in 10 classes, and their centred, normalised forms as float64"""
    if 'eval' not in CACHE:
        from dualvar_amd.utils.features import centre_normalise
        n_test, n_train, D, C = 130, 1000, 512, 10
        gen = torch.Generator().manual_seed(2024)
        te, tr = torch.randn((n_test, D), generator=gen).to(gpu), torch.randn((n_train, D), generator=gen).to(gpu)
        tel, trl = torch.randint(0, C, (n_test,), generator=gen), torch.randint(0, C, (n_train,), generator=gen)
        CACHE['eval'] = (te, tel, tr, trl, C, centre_normalise(te).double(), centre_normalise(tr).double())
    return CACHE['eval']
