"""mmdyn_bn_eval_swish_bwd on a real MI355X against PyTorch's own operators (ATen on the CPU, fp64): F.batch_norm(training=False)
+ Swish and its autograd -- one hop to what the reference runs under ``module.eval()`` (vae.py:200-208, 268-276).  Tolerances: relative
L2 < 1e-5 for dy, dgamma and dbeta, the figures of the train-mode pair in tests/test_kernels_aten_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from mmdyn_hip import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
EPS = 1e-5

# (G, rows_per_group, C): a ragged last 32-row tile (75 = 2 * 32 + 11); two groups with different statistics; every channel width of
# the stacks (8-channel threads: 8 ... 64 row lanes per block, so between four rows per thread and idle row lanes in a 32-row tile)
SHAPES = [(1, 75, 256), (2, 192, 128), (1, 1024, 64), (2, 3 * 1024, 32)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


_CASES = {}


def case(G, rpg, C):
    """Inputs and the fp64 ATen reference of one shape, computed once: group g normalises with its own running estimates."""
    key = (G, rpg, C)
    if key in _CASES:
        return _CASES[key]
    y, da = rnd(G, rpg, C, seed=1) * 2 + 0.3, rnd(G, rpg, C, seed=2)
    rm, rv = rnd(G, C, seed=3, scale=0.4), rnd(G, C, seed=4).abs() + 0.5
    gamma, beta = rnd(C, seed=5) + 1.5, rnd(C, seed=6)
    yd = y.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    us = [F.batch_norm(yd[g].t()[None], rm[g].double(), rv[g].double(), gd, bd, False, 0.0, EPS)[0].t() for g in range(G)]
    u = torch.stack(us)                                              # [G][rpg][C]
    a = u * torch.sigmoid(u)
    gy, gg, gb = torch.autograd.grad(a, (yd, gd, bd), da.double(), retain_graph=True)
    du = torch.autograd.grad(a, u, da.double())[0]                   # dL/du: what a fused GEMM epilogue hands over (da_is_du)
    mean, rstd = torch.empty(G, C, device=DEV), torch.empty(G, C, device=DEV)
    for g in range(G):                                               # per-group statistics through the product's own entry point
        ops.B.bn_eval_stats(rm[g].to(DEV), rv[g].to(DEV), mean[g:g + 1], rstd[g:g + 1], 1, C, EPS)
    out = dict(y=y.reshape(-1, C).to(DEV), da=da.reshape(-1, C).to(DEV), du=du.float().reshape(-1, C).to(DEV), mean=mean, rstd=rstd,
               gamma=gamma.to(DEV), beta=beta.to(DEV), gy=gy.reshape(-1, C), gg=gg, gb=gb)
    # dy from the fp32-rounded du (the da_is_du input): the same linear map in fp64
    out["gy_du"] = (out["du"].double().cpu().reshape(G, rpg, C) * (gamma.double() * torch.rsqrt(rv.double() + EPS))[:, None]).reshape(-1, C)
    _CASES.clear()
    _CASES[key] = out
    return out


def finalize(partial, G, rpg, C):
    T = ops.B.colstats_tiles(rpg)
    sums, dg, db = torch.empty(G, 2, C, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops.B.bn_bwd_finalize(partial, sums, dg, db, torch.empty(32, G, 2, C, dtype=torch.float64, device=DEV), G, T, C, 0.0)
    return dg, db


@pytest.mark.parametrize("G,rpg,C", SHAPES)
@pytest.mark.parametrize("da_is_du", [False, True])
def test_bn_eval_swish_bwd_against_aten(G, rpg, C, da_is_du):
    c = case(G, rpg, C)
    src, want = (c["du"], c["gy_du"]) if da_is_du else (c["da"], c["gy"])
    T = ops.B.colstats_tiles(rpg)
    args = (c["mean"], c["rstd"], c["gamma"], c["beta"])
    # without partial
    dy0 = torch.empty_like(c["y"])
    ops.B.bn_eval_swish_bwd(src, c["y"], *args, dy0, None, G, rpg, C, da_is_du)
    d = rel(dy0, want)
    print("dy rel L2", d)
    assert d < TOL
    # with partial: the same dy, and the table bn_bwd_finalize turns into dgamma / dbeta
    dy1, partial = torch.empty_like(c["y"]), torch.full((G, T, 2, C), float("nan"), device=DEV)
    ops.B.bn_eval_swish_bwd(src, c["y"], *args, dy1, partial, G, rpg, C, da_is_du)
    assert rel(dy1, want) < TOL and bool(torch.isfinite(partial).all())
    dg, db = finalize(partial, G, rpg, C)
    print("dgamma / dbeta rel L2", rel(dg, c["gg"]), rel(db, c["gb"]))
    assert rel(dg, c["gg"]) < TOL and rel(db, c["gb"]) < TOL
    # deterministic: a second launch writes the same table bit for bit
    again = torch.empty_like(partial)
    ops.B.bn_eval_swish_bwd(src, c["y"], *args, torch.empty_like(dy1), again, G, rpg, C, da_is_du)
    assert torch.equal(again, partial)
    # plane destination: the three planes sum to the fp32 destination bit for bit, with and without the fp32 copy
    for with_partial in (False, True):
        for keep in (True, False):
            d1, p = (torch.empty_like(c["y"]) if keep else None), ops.Planes(G * rpg, C, DEV)
            pt = torch.empty_like(partial) if with_partial else None
            ops.B.bn_eval_swish_bwd(src, c["y"], *args, d1, pt, G, rpg, C, da_is_du, planes=p)
            assert d1 is None or torch.equal(p.float(), d1)
            assert rel(p.float(), dy1 if with_partial else dy0) < 2e-7
            assert pt is None or torch.equal(pt, partial)
    if da_is_du:
        # y is not read: None gives the same result as a given y
        dy2 = torch.empty_like(dy0)
        ops.B.bn_eval_swish_bwd(src, None, *args, dy2, None, G, rpg, C, True)
        assert torch.equal(dy2, dy0)


def test_argument_errors_are_negative_codes_without_a_launch():
    lib = _lib.load()
    G, rpg, C = 1, 64, 32
    t = torch.zeros(G * rpg, C, device=DEV)
    s, v = torch.zeros(G, C, device=DEV), torch.zeros(C, device=DEV)
    part = torch.zeros(G, ops.B.colstats_tiles(rpg), 2, C, device=DEV)
    p = lambda x: None if x is None else x.data_ptr()
    call = lambda da, y, dy, dyp, partial, G_, r_, C_, is_du: lib.mmdyn_bn_eval_swish_bwd(
        p(da), p(y), p(s), p(s), p(v), p(v), p(dy), p(dyp), p(partial), G_, r_, C_, is_du, None)
    assert call(t, t, None, None, None, G, rpg, C, 0) < 0            # no destination
    assert call(None, t, t, None, None, G, rpg, C, 0) < 0            # no da
    assert call(t, None, t, None, None, G, rpg, C, 0) < 0            # swish'(u) needs y
    assert call(t, None, t, None, part, G, rpg, C, 1) < 0            # the sums need xhat, so y
    assert call(t, t, t, None, None, G, rpg, 48, 0) < 0              # 256 % (C / 4) != 0
    assert call(t, t, t, None, None, G, rpg, 512, 0) < 0
    assert call(t, t, t, None, None, 0, rpg, C, 0) < 0
    assert call(t, t, t, None, None, G, 0, C, 0) < 0
    assert lib.mmdyn_bn_eval_swish_bwd(p(t), p(t), None, p(s), p(v), p(v), p(t), None, None, G, rpg, C, 0, None) < 0
    assert float(t.abs().sum()) == 0.0                               # nothing was written
