"""The restatement the quantile tests compare against, shared by tests/test_quantiles_emu.py and tests/test_quantiles_gpu.py:
``torch.sort`` over the sample axis, the explicit NaN rule and single fp64 torch operations for the interpolation -- the contract of
mmdyn_ensemble_quantiles in include/mmdyn_hip.h, written without the engine -- and the host's (lo, frac) of a quantile, restated
independently of mmdyn_hip/engine.py (``divmod`` on the fp64 product instead of floor and a subtraction)."""
import numpy as np
import torch

from dirty import bits

QUANTILES_MAX = 8          # MMDYN_QUANTILES_MAX
QUANTILE_N_MAX = 128       # MMDYN_QUANTILE_N_MAX


def index_of(quantiles, N):
    """h = q (N - 1) in fp64 -> (lo, frac) per q: lo = floor(h), frac = h - lo; q = 1: (N - 1, 0)."""
    lo, frac = [], []
    for q in quantiles:
        whole, part = divmod(float(q) * float(N - 1), 1.0)
        assert 0 <= int(whole) <= N - 1 and 0.0 <= part < 1.0
        lo.append(int(whole))
        frac.append(part)
    return lo, frac


def restate(p, lo, frac):
    """p [N, ...] fp32 (any device) -> [Q, ...] fp32: s = sort(p) over axis 0; s[lo] where frac == 0, else
    fp32(s[lo] + frac * (s[hi] - s[lo])) with hi = min(lo + 1, N - 1), the difference, the product and the sum one fp64 torch
    operation each; an element with a NaN sample is NaN in all Q outputs."""
    N = p.shape[0]
    s = torch.sort(p, dim=0).values
    nan = torch.isnan(p).any(0)
    out = []
    for l, f in zip(lo, frac):
        if f == 0.0:
            r = s[l].clone()
        else:
            a, b = s[l].double(), s[min(l + 1, N - 1)].double()
            d = torch.sub(b, a)
            d = torch.mul(d, f)
            r = torch.add(a, d).to(torch.float32)
        out.append(torch.where(nan, torch.full_like(r, float("nan")), r))
    return torch.stack(out)


def neighbours(p, lo):
    """(s_lo, s_hi) per quantile, [Q, ...] each."""
    N = p.shape[0]
    s = torch.sort(p, dim=0).values
    return torch.stack([s[l] for l in lo]), torch.stack([s[min(l + 1, N - 1)] for l in lo])


def unsigned_zero(t):
    """-0.0 -> +0.0: the one thing the contract leaves open (values that compare equal are interchangeable)."""
    return torch.where(t == 0, torch.zeros_like(t), t)


def first_diff(a, b):
    """dirty.first_diff with the sign of a zero ignored."""
    ba, bb = bits(unsigned_zero(a)), bits(unsigned_zero(b))
    if ba.shape != bb.shape:
        return 0
    ne = (ba != bb).nonzero()
    return int(ne[0]) if ne.numel() else None


def textbook(p, quantiles):
    """numpy.quantile (``linear``) of the samples widened to fp64: [Q, ...] fp64."""
    return torch.from_numpy(np.quantile(p.double().cpu().numpy(), [float(q) for q in quantiles], axis=0))
