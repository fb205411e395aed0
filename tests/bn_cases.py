"""Per-element and per-channel checks for the fp32 BatchNorm + Swish kernels (csrc/bn.hip) and mmdyn_act_fwd / mmdyn_act_bwd
(csrc/elementwise.hip).  Shared by tests/test_bn_emu.py (CPU: the emulation, a plain torch-fp32 evaluation, wrong variants) and
tests/test_bn_gpu.py (HipBackend).  The exact column sums (family A) live in tests/exact_cases.py (run_colstats, run_eval_table).

B. Finalize from a given table (mmdyn_bn_finalize in both forms, mmdyn_bn_reduce_partials + mmdyn_bn_finalize_sums,
   mmdyn_bn_bwd_finalize / _sums): T is an argument, so the kernels are driven with synthetic fp32 partial tables.  Reference: fp64 on
   the table.  Bound per channel: 1/2 ulp32(ref) + d, d the propagated fp64 rounding of the written expression (`finalize_ref`).
C. Sums from data (mmdyn_colstats, mmdyn_bn_swish_bwd_reduce): the table summed over its tiles against fp64 sums per entry of
   [G][2][C], |got - ref| <= 2^-24 (D sum |t_r| + sum e_r), D the fp32 summation depth of colreduce_kernel (`depth`); then
   colstats -> bn_finalize against fp64 statistics of the data.
D. Element-wise outputs by store16_cases.check_rule with T = fp32, on inputs a norm cannot use (`hard_inputs`).
E. Argument errors (`run_argument_errors`, HipBackend only).

The constants c of family D are MEASURED as store16_cases.py measures its own: c = 4 x the largest |r32 - ref| / (2^-24 M) of a plain
torch-fp32 CPU evaluation over exactly the inputs below, rounded up (`python tests/bn_cases.py` prints the table; test_bn_emu.py
asserts it).  Elements whose reference is below the smallest normal are left out of the MEASUREMENT only (2^-24 M measures nothing
there); the check keeps them.  Every output of every launch sits in an exact_cases.Guarded buffer that is looked at afterwards.

A plain module, like tests/store16_cases.py; no fixture, no pytest setting.
"""
import math

import numpy as np
import torch

import exact_cases as X
import store16_cases as S
from dirty import bits
from mmdyn_hip import ops
from store16_cases import F32, F64, BF16, TWO_M24, check_rule, rne, ulp

EPS = float(np.float32(1e-5))          # the entry points take a float: the reference uses the value that arrives
MOM = float(np.float32(0.1))
OMM = float(np.float32(1.0) - np.float32(0.1))      # 1.f - momentum as the kernel forms it
TINY = 2.0 ** -126

# c per kernel: 4 x the largest value of the fp32 evaluation over all shapes and sign patterns below, rounded up (the measured maximum
# in the comment; measure() prints the table).  The inputs reach |u| = 100 and rstd = 316, where the constants of store16_cases.py
# (inputs within +-3) were not measured; the apply pass with da_is_du = 0 keeps the cancellation of swish' near u = -1.2785.
C_FWD = 21.0            # bn_swish_fwd: 5.08 ((2, 16447, 256))
C_APPLY = 3731.0        # bn_swish_bwd_apply, da_is_du = 0: 932.68 ((2, 16447, 256); 17 to 251 on the small shapes)
C_APPLY_DU = 16.0       # bn_swish_bwd_apply, da_is_du = 1: 3.77 ((2, 16447, 256))
C_EVAL = 852.0          # bn_eval_swish_bwd, da_is_du = 0: dy = da swish'(u) gamma rstd: 212.95 ((2, 16447, 256))
C_EVAL_DU = 8.0         # bn_eval_swish_bwd, da_is_du = 1: dy = du (gamma rstd): 1.97 ((2, 16447, 256))
C_ACT_FWD = 10.0        # act_fwd (Swish): 2.38 (n = 513 000)
C_ACT_BWD = 69.0        # act_bwd (Swish): 17.10 (n = 2 100 225: 1 - sigmoid(u) cancels for u of 10 to 17)
C_DU = 852.0            # du = da swish'(gamma xhat + beta) as the table of bn_eval_swish_bwd sums it, M = |da| x the largest intermediate
                        # of swish': 212.84 ((2, 16447, 256))
C_DU_SUMS = 53.0        # the same on the inputs of family C (bn_swish_bwd_reduce): 13.09 ((2, 16447, 256))

BN_SHAPES = S.BN_SHAPES
BIG = (2, 16447, 256)                                          # the eval kernel's tiling: 64-row tiles, a last tile of 63 rows, two groups
SUM_SHAPES = BN_SHAPES + [(1, 16385, 32), BIG, (1, 131073, 32)]
ACT_N = [1, 3, 4, 5, 1027, 513000, 2049 * 1025]                # the n % 4 tails; the last (> 4 x 2048 x 256): a second trip of the grid-stride loop
FINALIZE_CASES = [(1, 1, 32), (4, 5, 128), (2, 257, 64), (1, 512, 32), (3, 300, 256), (1, 640, 32), (1, 1000, 64)]      # G, T, C
CRAFTED_CASES = [(1, 640, 32), (2, 1000, 64)]                  # the table "crafted": T from 640 on, where bn_splits(T) exceeds 4
EVAL_VARIANTS = ("da", "du", "du_table", "da_table")           # NEED_Y without a table, !NEED_Y, PARTIAL (da_is_du = 1 / 0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uniform(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def guarded_like(t, dev, dtype=None):
    """A Guarded buffer that holds a copy of t ([rows][cols], or a vector as one row): an ACCUMULATOR in a guard band."""
    t2 = t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])
    gb = X.Guarded(t2.shape[0], t2.shape[1], dtype or t.dtype, dev)
    gb.t.copy_(t2.reshape(-1))
    return gb


def within(got, ref, bound, what, names=("group", "channel")):
    """|got - ref| <= bound per element of [rows][C] (a NaN fails); the failure names the element.  -> largest |err| / bound."""
    got, ref, bound = got.detach().cpu().double().reshape(ref.shape), ref.double(), bound.double().expand(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"{what}: largest |got - ref| / bound = {ratio:.3f}")
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        cols = ref.shape[-1]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} entries are outside their bound, the first at {names[0]} {i // cols}, "
                             f"{names[1]} {i % cols}: reference {ref.reshape(-1)[i].item()!r}, found {got.reshape(-1)[i].item()!r}, "
                             f"|difference| {err.reshape(-1)[i].item()!r} against {bound.reshape(-1)[i].item()!r}")
    return ratio


# ---- the tiling of the column reductions, restated (asserted against mmdyn_colstats_tiles wherever it is used) -------------------
def tile_rows_for(rpg):
    return min(max(rpg // 256 // 32 * 32, 32), 512)


def depth(be, rpg, C, per_thread=4):
    """D, the fp32 summation depth of one entry of the table: a thread of colreduce_kernel owns `per_thread` channels of every RL-th
    row of its tile, RL = 256 / (C / per_thread) row lanes, and adds its ceil(tile_rows / RL) terms one after the other (one rounding
    per add); thread `c` then adds the RL lane sums from LDS, again one after the other; + 1 for the rounding of the term itself.
    Each rounding is at most 2^-24 of the running sum, which is at most sum |t_r|: |error| <= 2^-24 D sum |t_r| to first order.
    The sum over the T tiles is formed by the test in fp64.  At most 512 / 4 + 4 + 1 = 133 over the admitted C (32 .. 256).
    per_thread = 8: the table of bn_eval_swish_bwd_kernel."""
    tr = tile_rows_for(rpg)
    assert -(-rpg // tr) == be.colstats_tiles(rpg), (rpg, tr, be.colstats_tiles(rpg))
    RL = 256 // (C // per_thread)
    return -(-tr // RL) + RL + 1


# ---- D: inputs a norm cannot use ------------------------------------------------------------------------------------------------
_HARD = {}


def hard_inputs(shape, pattern=0):
    """y, da [G rpg][C], mean / rstd [G][C], gamma / beta [C] (fp32): u = gamma xhat + beta within +-3 on most channels, to +-30 on
    every fifth, past +-100 on channel 7 (exp overflows fp32 at 88.7; past 104 even its denormal reciprocal is gone); gamma in two
    sign patterns, gamma of channel 3 exactly 0; statistics that differ per group; rstd = 1 / sqrt(1e-5) on every eighth channel."""
    key = (shape, pattern)
    if key not in _HARD:
        G, rpg, C = shape
        g = _gen(7100 + G * 1000003 + rpg * 1009 + C + 17 * pattern)
        c = torch.arange(C)
        wide, far = c % 5 == 4, c == 7
        amp = torch.where(far, torch.tensor(46.0), torch.where(wide, 10.5, 1.0) * (0.9 + 0.2 * torch.rand(C, generator=g)))
        gamma = torch.where((c + pattern) % 2 == 0, 1.0, -1.0) * amp
        gamma[3] = 0.0
        beta = _uniform(g, C) * torch.where(far, 8.0, torch.where(wide, 4.0, 0.5))
        mean = _uniform(g, G, C) * 0.5 * (1 + torch.arange(G))[:, None]
        rstd = _uniform(g, G, C).abs() * (1 + torch.arange(G))[:, None] + 0.6
        rstd[:, c % 8 == 1] = 1 / math.sqrt(1e-5)
        xh = _uniform(g, G, rpg, C) * 2.6
        y = (mean[:, None] + xh / rstd[:, None]).reshape(-1, C).contiguous()
        da = _uniform(g, G * rpg, C)
        _HARD[key] = (y, da, mean, rstd, gamma, beta)
    return _HARD[key]


def hard_u(shape, pattern=0):
    y, da, mean, rstd, gamma, beta = hard_inputs(shape, pattern)
    G, rpg, C = shape
    return (gamma.double() * S._xhat(y.double(), mean.double(), rstd.double(), G, rpg, C) + beta.double()).reshape(-1, C)


def assert_hard_ranges(shape, pattern=0):
    """On the reference alone: the ranges the doc string promises are reached (shapes with 63 rows or more)."""
    G, rpg, C = shape
    u = hard_u(shape, pattern)
    y, da, mean, rstd, gamma, beta = hard_inputs(shape, pattern)
    c = torch.arange(C)
    plain = (c % 5 != 4) & (c != 7)
    assert float(gamma[3]) == 0.0 and bool((gamma[c != 3] > 0).any()) and bool((gamma < 0).any())
    assert float(rstd.max()) == float(torch.tensor(1 / math.sqrt(1e-5)))
    assert float(u[:, plain].abs().max()) <= 3.8
    if G > 1:
        assert not torch.equal(mean[0], mean[1]) and not torch.equal(rstd[0], rstd[1])
    if G * rpg >= 63:
        assert float(u[:, 7].max()) > 104 and float(u[:, 7].min()) < -104
        wide = u[:, c % 5 == 4]
        assert float(wide.max()) > 25 and float(wide.min()) < -25 and float(wide.abs().max()) < 36


# ---- D: the formulas that store16_cases.py does not have ---------------------------------------------------------------------------
def f_eval(dt, y, da, mean, rstd, gamma, beta, G, rpg, C, da_is_du):
    """dy = du (gamma rstd), du = da swish'(gamma xhat + beta) or da itself -> (dy, M, underflow allowance, its mask), [G rpg][C]."""
    da, y, mean, rstd, gamma, beta = (t.to(dt) for t in (da, y, mean, rstd, gamma, beta))
    sc = (gamma * rstd)[:, None]
    d = da.reshape(G, rpg, C)
    if da_is_du:
        return (d * sc).reshape(-1, C), (d * sc).abs().reshape(-1, C), None, None
    u = gamma * S._xhat(y, mean, rstd, G, rpg, C) + beta
    U, low = underflow(u, d, sc.abs().double())
    return (d * S.swish_grad(u) * sc).reshape(-1, C), (d.abs() * S.swish_grad_mag(u) * sc.abs()).reshape(-1, C), U.reshape(-1, C), low.reshape(-1, C)


def f_du_mag(dt, y, da, mean, rstd, gamma, beta, G, rpg, C):
    """(du, M = |da| x the largest intermediate of swish', xhat, underflow allowance, its mask), [G][rpg][C]."""
    da, y, mean, rstd, gamma, beta = (t.to(dt) for t in (da, y, mean, rstd, gamma, beta))
    xh = S._xhat(y, mean, rstd, G, rpg, C)
    u = gamma * xh + beta
    d = da.reshape(G, rpg, C)
    return (d * S.swish_grad(u), d.abs() * S.swish_grad_mag(u), xh, *underflow(u, d))


def underflow(u, dh, scale=1.0):
    """fp32 has no sigmoid below its smallest normal: for u < -87.3 the reciprocal 1 / (1 + exp(-u)) is subnormal (2^-149 apart) or,
    on the device, flushed to zero, and exp(-u) itself overflows at 88.7 -- while dh swish'(u) = dh s (1 + u (1 - s)) is still a normal
    number (1e-37) down to u = -92.  M scales with s, so 2^-24 M measures nothing there (the case section V of docs/LAB_NOTES.md met in
    its dlogit).  Where the fp64 sigmoid is below 2^-125 such an element is left out of the MEASUREMENT, and the CHECK allows it the
    absolute error of a sigmoid flushed from the smallest normal, 2^-126 |dh| (1 + |u|) |scale|.  -> (that allowance, zero elsewhere;
    the mask)."""
    u, dh = u.double(), dh.double()
    low = S._sigmoid(u) < 2.0 ** -125
    return low * TINY * dh.abs() * (1 + u.abs()) * scale, low


def print_outside(got, ref, M, c, low, what):
    """The figure of the elements OUTSIDE the underflow zone (the rule itself is asserted on all of them by check_rule)."""
    ok = ~low.reshape(ref.shape)
    err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()[ok] / (0.5 * ulp(ref, F32) + c * TWO_M24 * M)[ok]
    print(f"{what}: largest |got - ref| / bound outside the underflow zone = {float(err.max()) if err.numel() else 0.0:.3f} "
          f"({int(low.sum())} elements inside)")


def with_underflow(M, U, c):
    """M for check_rule such that c 2^-24 M carries the absolute allowance U as well."""
    return M + U / (c * TWO_M24)


_LAST = {}


def last(key, fn):
    """fn() of the latest key (one slot: the fp64 references of the large shape are shared by the launches that follow each other)."""
    if _LAST.get("key") != key:
        _LAST["key"], _LAST["value"] = key, fn()
    return _LAST["value"]


# ---- D: runners -------------------------------------------------------------------------------------------------------------------
def run_fwd(be, dev, shape, pattern=0, figures=None):
    return S.run_fwd(be, dev, shape, F32, figures=figures, what=f"pattern {pattern}: ", inputs=hard_inputs(shape, pattern), c=C_FWD)


def run_apply(be, dev, shape, da_is_du, pattern=0, figures=None):
    return S.run_apply(be, dev, shape, F32, da_is_du, figures=figures, what=f"pattern {pattern}: ", inputs=hard_inputs(shape, pattern),
                       c=C_APPLY_DU if da_is_du else C_APPLY)


def run_act_bwd(be, dev, shape, act, figures=None):
    """store16_cases.run_act_bwd with T = fp32 (its own inputs, [G rpg][C]): Swish by the rule with the constant measured here, ReLU
    with `==`."""
    return S.run_act_bwd(be, dev, shape, F32, act, figures=figures, c=C_ACT_BWD)


def guarded_planes(rows, C, dev):
    """An ops.Planes whose tensor is a Guarded slice -> (Planes, Guarded)."""
    gb = X.Guarded(rows * 3, C, BF16, dev)
    p = ops.Planes.__new__(ops.Planes)
    p.t = gb.view(rows, 3, C)
    return p, gb


def split_ref(x):
    """The exact three-term bf16 split of x [rows][C] fp32 -> [rows][3][C] (ops.Planes): hi = bf16(x), mid = bf16(x - hi), lo the rest."""
    hi = x.to(BF16)
    r = x - hi.float()
    mid = r.to(BF16)
    return torch.stack((hi, mid, (r - mid.float()).to(BF16)), 1)


def run_eval(be, dev, shape, variant, dest, pattern=0, figures=None):
    """mmdyn_bn_eval_swish_bwd, one of the three instances of its kernel (EVAL_VARIANTS), dy alone / planes alone / both.  The fp32
    result by the rule; the plane tensor is the exact split of the launch's fp32 result (planes alone: of a value that passes the
    rule); the table, summed over its tiles, per entry against fp64 sums."""
    G, rpg, C = shape
    y, da, mean, rstd, gamma, beta = inp = hard_inputs(shape, pattern)
    is_du, table = variant.startswith("du"), variant.endswith("_table")
    c = C_EVAL_DU if is_du else C_EVAL
    ref, M0, U, low = last(("eval", shape, pattern, is_du), lambda: f_eval(F64, *inp, G, rpg, C, is_du))
    M = M0 if U is None else with_underflow(M0, U, c)
    T = be.colstats_tiles(rpg)
    dy = X.Guarded(G * rpg, C, F32, dev) if dest in ("dy", "both") else None
    pl, pg = guarded_planes(G * rpg, C, dev) if dest in ("planes", "both") else (None, None)
    P = X.Guarded(G * T * 2, C, F32, dev) if table else None
    be.bn_eval_swish_bwd(da.to(dev), None if (is_du and not table) else y.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), beta.to(dev),
                         None if dy is None else dy.view(G * rpg, C), None if P is None else P.view(G, T, 2, C), G, rpg, C, is_du, planes=pl)
    _sync(dev)
    what = f"pattern {pattern}: bn_eval_swish_bwd {shape} {variant} -> {dest}"
    out = None
    if dy is not None:
        dy.check(f"{what}: dy")
        out = check_rule(dy.values(), ref, M, F32, c, f"{what}: dy", figures)
        if low is not None:
            print_outside(dy.values(), ref, M0, c, low, f"{what}: dy")
    if pl is not None:
        pg.check(f"{what}: planes")
        pt = pl.t.detach().cpu()
        val = (pt[:, 0].float() + pt[:, 1].float()) + pt[:, 2].float()
        # (three bf16 terms hold an fp32 value exactly while the last one stays normal; bf16 ends at 2^-126, so below 2^-100 -- the
        #  gradients behind a saturated sigmoid -- the plane tensor is held to 2^-126 and the canonical split is not asked for)
        big = val.abs() >= 2.0 ** -100
        if dy is not None:
            X.check_exact(torch.where(big, val, 0.0), torch.where(big, dy.values(), 0.0), f"{what}: planes against dy", bitwise=True)
            within(val, dy.values().double(), torch.where(big, 0.0, 2.0 ** -126).double(), f"{what}: planes against dy, small values", ("row", "channel"))
        else:
            out = check_rule(val, ref, M + 2.0 ** -126 / (c * TWO_M24), F32, c, f"{what}: planes", figures)
        want = split_ref(val)
        X.check_exact(torch.where(big[:, None], pt, 0.0).reshape(-1, C), torch.where(big[:, None], want, 0.0).reshape(-1, C), f"{what}: the split")
    if table:
        P.check(f"{what}: partial")
        X._no_junk(P, f"{what}: partial")
        sums_check(P.values().double().reshape(G, T, 2, C).sum(1), inp, shape, depth(be, rpg, C, 8), is_du, f"{what}: partial", figures)
    return out


def sums_check(got, inp, shape, D, is_du, what, figures=None, c_du=C_DU):
    """got [G][2][C] = (sum du, sum du xhat) against fp64, per entry.  Terms t_r = du_r and du_r xhat_r; e_r, the term's own error: du
    carries c_du 2^-24 M (nothing with da_is_du: du is an input), and du xhat adds the two roundings of xhat and the one of the
    product, 2.5 x 2^-24 |du xhat|, rounded up into D + 3."""
    G, rpg, C = shape
    du, Mdu, xh, U, _ = f_du_mag(F64, *inp, G, rpg, C)
    Mdu = with_underflow(Mdu, U, c_du)
    if is_du:
        du, Mdu = inp[1].double().reshape(G, rpg, C), torch.zeros(G, rpg, C, dtype=F64)
    ref = torch.stack([du.sum(1), (du * xh).sum(1)], 1)
    absum = torch.stack([du.abs().sum(1), (du * xh).abs().sum(1)], 1)
    bound = TWO_M24 * (torch.stack([D * absum[:, 0], (D + 3) * absum[:, 1]], 1) + c_du * torch.stack([Mdu.sum(1), (Mdu * xh.abs()).sum(1)], 1))
    used = float(((got - ref).abs() / (TWO_M24 * absum).clamp_min(1e-300)).max())
    print(f"{what}: D = {D}, largest |got - ref| = {used:.3f} x 2^-24 sum |t|")
    r = within(got.reshape(-1, C), ref.reshape(-1, C), bound.reshape(-1, C), what, ("(group, sum)", "channel"))
    if figures is not None:
        figures.append((what, r, used))
    return r


def act_inputs(n):
    """u, dh [n]: u within +-3, to +-30 on every fifth element and to +-100 on every 97th; u[0] = +0 and, from n = 3 on, u[n / 2] = -0."""
    g = _gen(7300 + n)
    i = torch.arange(n)
    u = _uniform(g, n) * torch.where(i % 97 == 7, 100.0, torch.where(i % 5 == 4, 30.0, 3.0))
    u[0] = 0.0
    if n >= 3:
        u[n // 2] = -0.0
    return u, _uniform(g, n)


def run_act(be, dev, n, act, figures=None):
    """mmdyn_act_fwd and mmdyn_act_bwd on n elements: Swish by the rule; ReLU and the identity with `==` (the identity bit for bit)."""
    u, dh = act_inputs(n)
    w = max(d for d in range(1, min(n, 4096) + 1) if n % d == 0)      # (the flat tensor as [n / w][w]: guard bands of 64 x w elements)
    u, dh = u.reshape(-1, w), dh.reshape(-1, w)
    h, du = X.Guarded(n // w, w, F32, dev), X.Guarded(n // w, w, F32, dev)
    be.act_fwd(u.to(dev), h.view(n), act)
    be.act_bwd(dh.to(dev), u.to(dev), du.view(n), act)
    _sync(dev)
    what = f"act n={n} act={act}"
    h.check(f"{what}: h")
    du.check(f"{what}: du")
    if act == 1:
        if n >= 1027:
            assert float(u.max()) > 89 and float(u.min()) < -89
        ref, M0 = S.f_act_bwd(F64, dh, u)
        U, low = underflow(u, dh)
        out = (check_rule(h.values(), *S.f_swish_out(F64, u), F32, C_ACT_FWD, f"{what}: h", figures),
               check_rule(du.values(), ref, with_underflow(M0, U, C_ACT_BWD), F32, C_ACT_BWD, f"{what}: du", figures))
        print_outside(du.values(), ref, M0, C_ACT_BWD, low, f"{what}: du")
        return out
    X.check_exact(h.values(), u.clamp_min(0) if act == 2 else u, f"{what}: h", bitwise=act == 0)
    X.check_exact(du.values(), dh * (u > 0) if act == 2 else dh, f"{what}: du", bitwise=act == 0)


def run_eval_stats(be, dev, G, C):
    """mmdyn_bn_eval_stats: mean copies running_mean for every group; rstd within 1 ulp32 of 1 / sqrt(rv + eps), rv = 0 included."""
    g = _gen(7400 + G * 1000 + C)
    rm, rv = _uniform(g, C) * 3, torch.rand(C, generator=g) * 10.0 ** torch.randint(-6, 3, (C,), generator=g)
    rv[::5] = 0.0
    mean, rstd = X.Guarded(G, C, F32, dev), X.Guarded(G, C, F32, dev)
    be.bn_eval_stats(rm.to(dev), rv.to(dev), mean.view(G, C), rstd.view(G, C), G, C, 1e-5)
    _sync(dev)
    what = f"bn_eval_stats G={G} C={C}"
    mean.check(f"{what}: mean")
    rstd.check(f"{what}: rstd")
    X.check_exact(mean.values(), rm[None].expand(G, C), f"{what}: mean", bitwise=True)
    ref = (1 / torch.sqrt(rv.double() + EPS))[None].expand(G, C)
    return within(rstd.values(), ref, ulp(ref, F32), f"{what}: rstd")


# ---- D: the fp32 twin ---------------------------------------------------------------------------------------------------------------
def d_cases():
    """(shape, pattern) of the element-wise tests: both sign patterns on BN_SHAPES, pattern 0 on the large shape."""
    return [(s, p) for s in BN_SHAPES for p in (0, 1)] + [(BIG, 0)]


def twins():
    """(name, name of its constant, r32, ref, M[, mask of the elements left out: `underflow`]) of a plain torch-fp32 evaluation of
    every formula of family D over the tests' own inputs."""
    out = []
    for shape, p in d_cases():
        inp = hard_inputs(shape, p)
        y, da, mean, rstd, gamma, beta = inp
        tag = f"{shape} pattern {p}"
        out.append((f"fwd {tag}", "C_FWD", S.f_fwd(F32, y, mean, rstd, gamma, beta, *shape)[0], *S.f_fwd(F64, y, mean, rstd, gamma, beta, *shape)))
        sums = S.f_reduce(F64, da, y, mean, rstd, gamma, beta, *shape).float()
        for is_du in (False, True):
            out.append((f"apply {tag} da_is_du={int(is_du)}", "C_APPLY_DU" if is_du else "C_APPLY",
                        S.f_apply(F32, da, y, mean, rstd, gamma, beta, sums, *shape, is_du)[0], *S.f_apply(F64, da, y, mean, rstd, gamma, beta, sums, *shape, is_du)))
            e = f_eval(F64, *inp, *shape, is_du)
            out.append((f"eval {tag} da_is_du={int(is_du)}", "C_EVAL_DU" if is_du else "C_EVAL", f_eval(F32, *inp, *shape, is_du)[0], e[0], e[1], e[3]))
        e = f_du_mag(F64, *inp, *shape)
        out.append((f"du {tag}", "C_DU", f_du_mag(F32, *inp, *shape)[0], e[0], e[1], e[4]))
    for shape in SUM_SHAPES:
        inp = S.bn_inputs(shape, F32)
        e = f_du_mag(F64, *inp, *shape)
        out.append((f"du {shape} (sums)", "C_DU_SUMS", f_du_mag(F32, *inp, *shape)[0], e[0], e[1], e[4]))
    for shape in BN_SHAPES:
        u, dh = S.bn_inputs(shape, F32)[:2]
        out.append((f"act_bwd {shape}", "C_ACT_BWD", S.f_act_bwd(F32, dh, u)[0], *S.f_act_bwd(F64, dh, u)))
    for n in ACT_N:
        u, dh = act_inputs(n)
        out.append((f"act_fwd n={n}", "C_ACT_FWD", S.f_swish_out(F32, u)[0], *S.f_swish_out(F64, u)))
        out.append((f"act_bwd n={n}", "C_ACT_BWD", S.f_act_bwd(F32, dh, u)[0], *S.f_act_bwd(F64, dh, u), underflow(u, dh)[1]))
    return out


_TWIN = []


def twin_figures():
    """[(name, name of its constant, largest |r32 - ref| / (2^-24 M) over the elements with a normal reference)], computed once."""
    if not _TWIN:
        for name, c, r32, ref, M, *low in twins():
            ok = (M > 0) & (ref.abs() >= TINY)
            if low and low[0] is not None:
                ok &= ~low[0].reshape(ok.shape)
            _TWIN.append((name, c, float(((r32.double() - ref).abs()[ok] / (TWO_M24 * M[ok])).max()) if bool(ok.any()) else 0.0))
    return _TWIN


def worst_figures():
    worst = {}
    for _, key, ratio in twin_figures():
        worst[key] = max(worst.get(key, 0.0), ratio)
    return worst


def measure():
    for name, key, ratio in twin_figures():
        print(f"{name:60s} {key:10s} = {globals()[key]:7.1f}  measured {ratio:8.2f}")
    for key, v in worst_figures().items():
        print(f"{key:12s} largest {v:8.2f}  -> c = {math.floor(4 * v) + 1}")


# ---- B: finalize from a given table -------------------------------------------------------------------------------------------------
def rows_for(T, kind=None):
    """rows per group handed to the finalize with a T-tile table (the kernel trusts T; any n > 0 serves).  "crafted": a power of
    two, so that the division of the mean is exact."""
    if kind == "crafted":
        return 16384
    return 17 if T == 1 else 32 * T - 7


def bn_splits(T):
    """Slices of the tile sums in the two-launch form (csrc/bn.hip)."""
    return min(max(T // 128, 1), 32)


def tile_sum_sim(col, S):
    """One column of a table (T fp32 entries) summed in fp64 in the order of tile_sum_kernel with S slices followed by the finish
    kernels: slice s owns the tiles [s per, (s + 1) per), per = ceil(T / S); its eight threads of a channel add every eighth tile
    one after the other, neighbours are paired (the shuffle), the four pairs are added in order, and the slices are added in order."""
    T = len(col)
    per = -(-T // S)
    total = 0.0
    for s in range(S):
        lane = []
        for tl in range(8):
            a = 0.0
            for t in range(s * per + tl, min(T, (s + 1) * per), 8):
                a += float(col[t])
            lane.append(a)
        r = 0.0
        for k in range(4):
            r += lane[2 * k] + lane[2 * k + 1]
        total += r
    return total


_TABLES = {}


def table(kind, G, T, C):
    """A synthetic partial table [G][T][2][C] fp32: per tile (sum y, sum y^2).
    "well": moments of well-conditioned channels (|mean| <= std .. 1.5 std).
    "edge": per channel one of -- constant data (c % 3 == 0; the tile sums are rounded to fp32, so sum y^2 / n - m^2 is zero or
        slightly off it; on c % 6 == 0 the squares are pushed below by 2^-20, which makes it negative, on channel 6 by more than eps),
        mean / std = 100 (c % 3 == 1), mean / std = 1000 (c % 3 == 2).
    "spread": entries over 41 binades, so that fp64 addition rounds and the grouping of the tile sums can show; the first sum in both
        signs and scaled by 2^-6, the second positive.  (It shows in fp64 only: the fp32 outputs round the difference away.)
    "crafted" (T >= 640): a column whose fp32 RESULT depends on the grouping.  Tiles 0 and 8 hold 1 and 2^-24 -- an fp32 rounding
        tie -- and four tiles of one thread of the two-launch form's second slice hold 2^-54 each: added together first they are one
        fp64 ulp of 1 and break the tie upwards (1 + 2^-23); added one by one onto 1 + 2^-24, as a four-slice sum does whose first
        slice still holds them, each is lost and the tie goes to even (1.0).  Both are within the bound; only one is the
        two-launch form's."""
    key = (kind, G, T, C)
    if key not in _TABLES and kind == "crafted":
        per = -(-T // bn_splits(T))
        t0 = -(-per // 8) * 8
        assert bn_splits(T) > 4 and t0 + 24 < min(2 * per, -(-T // 4)) and per > 8
        t = torch.zeros(G, T, 2, C, dtype=F64)
        t[:, 0, 0], t[:, 8, 0], t[:, 0, 1] = 1.0, 2.0 ** -24, 4.0
        t[:, t0:t0 + 25:8, 0] = 2.0 ** -54
        _TABLES[key] = t.float().contiguous()
    if key not in _TABLES:
        g = _gen(7500 + G * 100003 + T * 1009 + C + {"well": 0, "edge": 1, "spread": 2}[kind])
        n = rows_for(T)
        r = torch.full((T,), 32.0, dtype=F64)
        r[-1] = n - (32 if T > 1 else 0) * (T - 1)
        r = r[None, :, None]
        if kind == "spread":
            a = X.arbitrary((G, T, 2, C), 7600 + G + T + C, binades=20).double()
            t = torch.stack([a[:, :, 0] * 2.0 ** -6, a[:, :, 1].abs()], 2)
        else:
            c = torch.arange(C)
            sd = (torch.rand(G, 1, C, generator=g) + 0.5).double()
            if kind == "well":
                mu = _uniform(g, G, 1, C).double() * sd * 1.5
            else:
                mu = torch.where((c % 3 == 1)[None, None], 100.0, 1000.0) * sd
                sd = torch.where((c % 3 == 0)[None, None], 0.0, sd)
                mu = torch.where((c % 3 == 0)[None, None], torch.where(c == 6, 8.0, 0.1 * (c + 2)).double()[None, None], mu)
            noise = lambda: 1 + 0.05 * _uniform(g, G, T, C).double() * (sd > 0)
            s1 = r * mu * (noise() if kind == "well" else 1.0)
            s2 = r * (sd * sd * noise() + mu * mu)
            if kind == "edge":
                s2 = s2.float().double() * torch.where((c % 6 == 0)[None, None], 1 - 2.0 ** -20, 1.0)
            t = torch.stack([s1, s2], 2)
        _TABLES[key] = t.float().contiguous()
    return _TABLES[key]


def finalize_ref(tab, n, repeat, rm0, rv0):
    """fp64 on the table -> dict of (reference, bound) per output.  Written expression (bn_stats_finish_channel): S = sum of the T
    fp32 entries in fp64, m = S1 / n, var = max(S2 / n - m^2, 0), rstd = 1 / sqrt(var + eps), unb = var n / (n - 1), and per group
    in order, `repeat` times, r <- (1 - mom) r + mom fp32(x) in fp32.
    d, the fp64 rounding the kernel may add against this reference (u = 2^-53, A = sum of |entries|):
      sums: at most T - 1 adds in any grouping, each within u of a partial sum <= A:            d_S   = T u A
      m = S1 / n: + one division:                                                               d_m   = (T + 1) u A1 / n
      var: S2 / n, m^2, the subtraction (3 roundings of values <= A2 / n + m^2) + the inputs:    d_var = (T + 4) u (A2 / n + m^2) + 2 |m| d_m
           (the clamp is 1-Lipschitz); relative to var + eps this is the issue's 2^-50 (S2 / n) / (var + eps) order
      rstd: |d rstd / d var| = rstd^3 / 2, + the add, sqrt and division:                         d_r   = rstd^3 d_var / 2 + 3 u rstd
      unb: + two roundings:                                                                      d_unb = (d_var + 2 u var) n / (n - 1)
    all doubled for what first order leaves out.  On the well-conditioned tables d is 1e-13 relative, nothing against 2^-24.
    running_*: every EMA step adds two fp32 roundings (a product, then the fused multiply-add), each at most half an ulp of the
    largest intermediate: 2 G repeat half-ulps; the fp32(x) it reads may sit one step off where d straddles a rounding boundary
    (`flip`, zero otherwise)."""
    G, T, _, C = tab.shape
    u = 2.0 ** -53
    t = tab.double()
    Ssum, A = t.sum(1), t.abs().sum(1)
    m = Ssum[:, 0] / n
    raw = Ssum[:, 1] / n - m * m
    var = raw.clamp_min(0)
    rstd = 1 / torch.sqrt(var + EPS)
    fac = n / (n - 1 if n > 1 else 1)
    unb = var * fac
    d_m = 2 * (T + 1) * u * A[:, 0] / n
    d_var = 2 * ((T + 4) * u * (A[:, 1] / n + m * m) + 2 * m.abs() * d_m)
    d_r = rstd ** 3 * d_var / 2 + 6 * u * rstd
    d_unb = (d_var + 4 * u * var) * fac
    half = lambda x: 0.5 * ulp(x, F32)
    out = {"mean": (m, half(m) + d_m), "rstd": (rstd, half(rstd) + d_r), "var": var, "raw": raw, "sums": Ssum, "A": A}
    for name, x, d, r0 in (("running_mean", m, d_m, rm0), ("running_var", unb, d_unb, rv0)):
        if r0 is None:
            continue
        r, big, flip = r0.double().clone(), torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
        for g in range(G):
            x32 = rne(x[g], F32)
            flip = flip + (rne(x[g] + d[g], F32) - rne(x[g] - d[g], F32)).abs()
            for _ in range(repeat):
                a, b = OMM * r, MOM * x32
                r = a + b
                big = torch.maximum(big, torch.maximum(torch.maximum(a.abs(), b.abs()), r.abs()))
        out[name] = (r[None], (half(r) + 2 * G * repeat * half(big) + flip)[None])
    return out


def _forms(be, ticket):
    """Switch HipBackend between the two-launch and the ticket form (as test_single_launch_finalize_equals_two_launches does);
    the emulation has one form."""
    if hasattr(be, "force_ticket"):
        be.force_ticket, be.ticket_max_work = ticket, (1 << 30) if ticket else 0


def launch_finalize(be, dev, tab, n, repeat, running, ticket, what):
    """One mmdyn_bn_finalize launch, every output and the scratch guarded -> dict of CPU tensors."""
    G, T, _, C = tab.shape
    g = _gen(7700 + G + T + C)
    rm0, rv0 = (_uniform(g, C) * 2, torch.rand(C, generator=g) * 3 + 0.1) if running else (None, None)
    mean, rstd = X.Guarded(G, C, F32, dev), X.Guarded(G, C, F32, dev)
    scratch = X.Guarded(32 * G * 2, C, F64, dev)
    rm, rv = (guarded_like(rm0, dev), guarded_like(rv0, dev)) if running else (None, None)
    nbt = guarded_like(torch.tensor([[41]], dtype=torch.int64), dev) if running else None
    rule = (getattr(be, "force_ticket", None), getattr(be, "ticket_max_work", None))
    _forms(be, ticket)
    try:
        be.bn_finalize(tab.to(dev), mean.view(G, C), rstd.view(G, C), rm and rm.view(C), rv and rv.view(C), nbt and nbt.view(1),
                       scratch.view(32, G, 2, C), G, T, C, n, 1e-5, 0.1, repeat)
        _sync(dev)
    finally:
        if rule[0] is not None:
            be.force_ticket, be.ticket_max_work = rule
    out = {}
    for name, gb in (("mean", mean), ("rstd", rstd), ("scratch", scratch), ("running_mean", rm), ("running_var", rv), ("nbt", nbt)):
        if gb is not None:
            gb.check(f"{what}: {name}")
            out[name] = gb.values()
    out["rm0"], out["rv0"] = rm0, rv0
    return out


def check_finalize(out, tab, n, repeat, what, figures=None):
    G, T, _, C = tab.shape
    ref = finalize_ref(tab, n, repeat, out["rm0"], out["rv0"])
    for name in ("mean", "rstd", "running_mean", "running_var"):
        if name in out:
            r = within(out[name], *ref[name], f"{what}: {name}", ("group" if name in ("mean", "rstd") else "row", "channel"))
            if figures is not None:
                figures.append((f"{what}: {name}", r, None))
    if "nbt" in out:
        assert int(out["nbt"][0, 0]) == 41 + G * repeat, f"{what}: num_batches_tracked {int(out['nbt'][0, 0])}, expected {41 + G * repeat}"
    return ref


def assert_table(kind, tab, n):
    """Preconditions of a table, on the reference alone."""
    ref = finalize_ref(tab, n, 1, None, None)
    C = tab.shape[-1]
    c = torch.arange(C)
    if kind == "well":
        assert bool((ref["sums"][:, 1] / n <= 2.0 ** 10 * ref["var"]).all())
        assert float((ref["mean"][1] / ulp(ref["mean"][0], F32)).max()) < 0.5 + 1e-4        # d is nothing to fp32 precision
    if kind == "edge":
        const = ref["raw"][:, c % 3 == 0]
        assert float(const.abs().max()) < 1e-3 and bool((const < 0).any())
        if C > 6:
            assert float(ref["raw"][:, 6].max()) < -EPS          # without the clamp: the square root of a negative number
        ratio = ref["mean"][0].abs() / torch.sqrt(ref["var"])
        assert bool((ratio[:, c % 3 == 1] > 50).all()) and bool((ratio[:, c % 3 == 2] > 500).all())
    if kind == "spread":
        e = torch.floor(torch.log2(tab.abs().double()))
        assert float(e.max() - e.min()) >= 40
    if kind == "crafted":       # (in the kernels' order: the two-launch form's slices break the tie upwards, four slices do not)
        col, T = tab[0, :, 0, 0], tab.shape[1]
        a, b = tile_sum_sim(col, bn_splits(T)), tile_sum_sim(col, 4)
        assert a == 1 + 2.0 ** -24 + 2.0 ** -52 and b == 1 + 2.0 ** -24
        assert float(torch.tensor(a, dtype=F64).float()) == 1 + 2.0 ** -23 and float(torch.tensor(b, dtype=F64).float()) == 1.0


def run_finalize(be, dev, case, kind, repeat, running, figures=None):
    """mmdyn_bn_finalize in both forms against the fp64 reference; the two forms bit for bit on every output (tables "well" and
    "spread"; on "edge" too, it costs nothing)."""
    G, T, C = case
    n, tab = rows_for(T, kind), table(kind, *case)
    assert_table(kind, tab, n)
    outs = []
    for ticket in (False, True):
        what = f"bn_finalize {case} {kind} repeat={repeat} running={int(running)} {'ticket' if ticket else 'two launches'}"
        outs.append(launch_finalize(be, dev, tab, n, repeat, running, ticket, what))
        check_finalize(outs[-1], tab, n, repeat, what, figures)
    for name in ("mean", "rstd", "running_mean", "running_var", "nbt"):
        if name in outs[0]:
            X.check_exact(outs[1][name], outs[0][name], f"bn_finalize {case} {kind} repeat={repeat}: {name}, ticket form against two launches", bitwise=True)


def run_finalize_sums(be, dev, case, kind):
    """mmdyn_bn_reduce_partials + mmdyn_bn_finalize_sums: the bits of mmdyn_bn_finalize (two launches) from the same table and n;
    with the sums and n doubled, mean and rstd do not move."""
    G, T, C = case
    n, tab = rows_for(T), table(kind, *case)
    what = f"bn_finalize_sums {case} {kind}"
    base = launch_finalize(be, dev, tab, n, 2, True, False, f"{what}: bn_finalize")
    sums, scratch = X.Guarded(G * 2, C, F64, dev), X.Guarded(32 * G * 2, C, F64, dev)
    be.bn_reduce_partials(tab.to(dev), sums.view(G, 2, C), scratch.view(32, G, 2, C), G, T, C)
    _sync(dev)
    sums.check(f"{what}: sums")
    scratch.check(f"{what}: scratch")
    ref = finalize_ref(tab, n, 1, None, None)
    within(sums.values().reshape(G * 2, C), ref["sums"].reshape(G * 2, C), (2 * T * 2.0 ** -53 * ref["A"]).reshape(G * 2, C), f"{what}: sums",
           ("(group, sum)", "channel"))
    for scale in (1, 2):
        mean, rstd = X.Guarded(G, C, F32, dev), X.Guarded(G, C, F32, dev)
        rm, rv = guarded_like(base["rm0"], dev), guarded_like(base["rv0"], dev)
        nbt = guarded_like(torch.tensor([[41]], dtype=torch.int64), dev)
        s = (sums.values() * scale).reshape(G, 2, C).to(dev)
        run = scale == 1
        be.bn_finalize_sums(s, mean.view(G, C), rstd.view(G, C), rm.view(C) if run else None, rv.view(C) if run else None,
                            nbt.view(1) if run else None, G, C, n * scale, 1e-5, 0.1, 2)
        _sync(dev)
        names = (("mean", mean), ("rstd", rstd)) + ((("running_mean", rm), ("running_var", rv), ("nbt", nbt)) if run else ())
        for name, gb in names:
            gb.check(f"{what} x{scale}: {name}")
            X.check_exact(gb.values(), base[name], f"{what}, sums and n x {scale}: {name} against bn_finalize", bitwise=True)


def bwd_ref(tab):
    t = tab.double()
    return t.sum(1), t.abs().sum(1)


def run_bwd_finalize(be, dev, case, kind, figures=None):
    """mmdyn_bn_bwd_finalize in both forms, beta_acc 0 (on JUNK-filled dgamma / dbeta: not read), 1 and 0.5 (on known values), null
    gradients; mmdyn_bn_bwd_finalize_sums with sums_scale 1 and 0.5, null sums_f / null gradients.  sums [G][2][C], dbeta = sum over
    the groups of sums[:, 0], dgamma of sums[:, 1]: against fp64 sums of the table to 1/2 ulp32 + the fp64 rounding d = 2 T u A
    (finalize_ref), the accumulating forms + the rounding of the added term."""
    G, T, C = case
    tab = table(kind, *case)
    Ssum, A = bwd_ref(tab)
    d = 2 * T * 2.0 ** -53 * A
    half = lambda x: 0.5 * ulp(x, F32)
    g = _gen(7800 + G + T + C)
    old = {"dgamma": _uniform(g, C), "dbeta": _uniform(g, C) * 4}
    tot = {"dbeta": (Ssum[:, 0].sum(0), d[:, 0].sum(0)), "dgamma": (Ssum[:, 1].sum(0), d[:, 1].sum(0))}
    rule = (getattr(be, "force_ticket", None), getattr(be, "ticket_max_work", None))
    keep = {}
    for ticket in (False, True):
        for beta_acc, grads in ((0.0, True), (1.0, True), (0.5, True), (0.0, False)):
            what = f"bn_bwd_finalize {case} {kind} beta_acc={beta_acc} grads={int(grads)} {'ticket' if ticket else 'two launches'}"
            sums, scratch = X.Guarded(G * 2, C, F32, dev), X.Guarded(32 * G * 2, C, F64, dev)
            gr = {k: (guarded_like(v, dev) if beta_acc else X.Guarded(1, C, F32, dev)) for k, v in old.items()} if grads else {}
            _forms(be, ticket)
            try:
                be.bn_bwd_finalize(tab.to(dev), sums.view(G, 2, C), gr["dgamma"].view(C) if grads else None, gr["dbeta"].view(C) if grads else None,
                                   scratch.view(32, G, 2, C), G, T, C, beta_acc)
                _sync(dev)
            finally:
                if rule[0] is not None:
                    be.force_ticket, be.ticket_max_work = rule
            sums.check(f"{what}: sums")
            scratch.check(f"{what}: scratch")
            r = within(sums.values(), Ssum.reshape(G * 2, C), (half(Ssum) + d).reshape(G * 2, C), f"{what}: sums", ("(group, sum)", "channel"))
            if figures is not None:
                figures.append((f"{what}: sums", r, None))
            outs = [sums.values()]
            for k in gr:
                gr[k].check(f"{what}: {k}")
                s, ds = tot[k]
                ref = beta_acc * old[k].double() + s
                extra = half(s) + ds if beta_acc else ds             # (beta_acc = 1, 0.5: the product is exact, the added term is rounded once)
                within(gr[k].values(), ref[None], (half(ref) + extra)[None], f"{what}: {k}", ("row", "channel"))
                outs.append(gr[k].values())
            if ticket:
                for a, b in zip(outs, keep[(beta_acc, grads)]):
                    X.check_exact(a, b, f"{what}: against the two-launch form", bitwise=True)
            else:
                keep[(beta_acc, grads)] = outs
    # the synchronised form: fp64 sums in, sums_scale 1 / 0.5, null sums_f / null gradients
    s64 = Ssum.to(dev)
    for scale, with_f, grads in ((1.0, True, True), (0.5, True, True), (1.0, False, True), (0.5, True, False)):
        what = f"bn_bwd_finalize_sums {case} {kind} sums_scale={scale} sums_f={int(with_f)} grads={int(grads)}"
        sf = X.Guarded(G * 2, C, F32, dev) if with_f else None
        gr = {k: guarded_like(v, dev) for k, v in old.items()} if grads else {}
        be.bn_bwd_finalize_sums(s64, sf.view(G, 2, C) if with_f else None, gr["dgamma"].view(C) if grads else None,
                                gr["dbeta"].view(C) if grads else None, G, C, scale, 1.0)
        _sync(dev)
        if with_f:
            sf.check(f"{what}: sums_f")
            X.check_exact(sf.values(), rne(Ssum * scale, F32).reshape(G * 2, C), f"{what}: sums_f")
        for k in gr:
            gr[k].check(f"{what}: {k}")
            s = tot[k][0]
            ref = old[k].double() + s
            within(gr[k].values(), ref[None], (half(ref) + half(s) + 2 * G * 2.0 ** -53 * s.abs())[None], f"{what}: {k}", ("row", "channel"))


# ---- C: sums from data ----------------------------------------------------------------------------------------------------------------
def run_colstats(be, dev, shape, figures=None):
    """mmdyn_colstats on real values: per entry of [G][2][C], terms y_r (exact) and y_r^2 (one rounding: e_r = 2^-24 y_r^2)."""
    G, rpg, C = shape
    y = S.bn_inputs(shape, F32)[0]
    T, D = be.colstats_tiles(rpg), depth(be, rpg, C)
    P = X.Guarded(G * T * 2, C, F32, dev)
    be.colstats(y.to(dev), P.view(G, T, 2, C), G, rpg, C)
    _sync(dev)
    what = f"colstats {shape}"
    P.check(what)
    X._no_junk(P, what)
    r = y.double().reshape(G, rpg, C)
    ref, absum = torch.stack([r.sum(1), (r * r).sum(1)], 1), torch.stack([r.abs().sum(1), (r * r).sum(1)], 1)
    bound = TWO_M24 * torch.stack([D * absum[:, 0], (D + 1) * absum[:, 1]], 1)
    got = P.values().double().reshape(G, T, 2, C).sum(1)
    used = float(((got - ref).abs() / (TWO_M24 * absum)).max())
    print(f"{what}: D = {D}, largest |got - ref| = {used:.3f} x 2^-24 sum |t|")
    ratio = within(got.reshape(-1, C), ref.reshape(-1, C), bound.reshape(-1, C), what, ("(group, sum)", "channel"))
    if figures is not None:
        figures.append((what, ratio, used))
    return ratio


def run_reduce(be, dev, shape, figures=None):
    """mmdyn_bn_swish_bwd_reduce in fp32: per entry of [G][2][C] (sums_check)."""
    G, rpg, C = shape
    inp = S.bn_inputs(shape, F32)
    y, da, mean, rstd, gamma, beta = inp
    T = be.colstats_tiles(rpg)
    P = X.Guarded(G * T * 2, C, F32, dev)
    be.bn_swish_bwd_reduce(da.to(dev), y.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), beta.to(dev), P.view(G, T, 2, C), G, rpg, C)
    _sync(dev)
    what = f"bn_swish_bwd_reduce {shape}"
    P.check(what)
    X._no_junk(P, what)
    return sums_check(P.values().double().reshape(G, T, 2, C).sum(1), inp, shape, depth(be, rpg, C), False, what, figures, C_DU_SUMS)


_STATS = {}


def stats_inputs(shape):
    """y [G rpg][C] = m + s z, z uniform: well-conditioned channels (|m| <= s), channel 1 with mean / std = 100, channel 2 with 1000;
    m and s differ per group."""
    if shape not in _STATS:
        G, rpg, C = shape
        g = _gen(7900 + G * 1000003 + rpg * 1009 + C)
        s = (torch.rand(G, 1, C, generator=g) + 0.5) * (1 + torch.arange(G))[:, None, None]
        m = _uniform(g, G, 1, C) * s
        m[:, :, 1], m[:, :, 2] = 100 * s[:, :, 1] / math.sqrt(3), 1000 * s[:, :, 2] / math.sqrt(3)
        _STATS[shape] = (m + s * _uniform(g, G, rpg, C)).reshape(-1, C).contiguous()
    return _STATS[shape]


def run_statistics(be, dev, shape, figures=None):
    """colstats -> bn_finalize against fp64 statistics of the data: mean within 2^-24 D E|y|, rstd within the first-order propagation
    1/2 rstd^3 2^-24 D (E y^2 + 2 |m| E|y|) + half an ulp.  On the channels with mean / std = 100 and 1000 the bound is loose by
    construction (single-pass variance): the test documents that conditioning, it does not fix it."""
    G, rpg, C = shape
    y = stats_inputs(shape)
    T, D = be.colstats_tiles(rpg), depth(be, rpg, C)
    P, mean, rstd = X.Guarded(G * T * 2, C, F32, dev), X.Guarded(G, C, F32, dev), X.Guarded(G, C, F32, dev)
    scratch = X.Guarded(32 * G * 2, C, F64, dev)
    be.colstats(y.to(dev), P.view(G, T, 2, C), G, rpg, C)
    be.bn_finalize(P.view(G, T, 2, C), mean.view(G, C), rstd.view(G, C), None, None, None, scratch.view(32, G, 2, C), G, T, C, rpg, 1e-5, 0.1, 1)
    _sync(dev)
    what = f"colstats -> bn_finalize {shape}"
    for name, gb in (("partial", P), ("mean", mean), ("rstd", rstd), ("scratch", scratch)):
        gb.check(f"{what}: {name}")
    r = y.double().reshape(G, rpg, C)
    m, Ea, E2 = r.mean(1), r.abs().mean(1), (r * r).mean(1)
    var = ((r - m[:, None]) ** 2).mean(1)
    ref = 1 / torch.sqrt(var + EPS)
    if rpg >= 63:
        ratio = m.abs() / var.sqrt()
        assert float(ratio[:, 1].min()) > 90 and float(ratio[:, 2].min()) > 900 and float(ratio[:, 3:].max()) < 2.5
    a = within(mean.values(), m, TWO_M24 * D * Ea, f"{what}: mean")
    b = within(rstd.values(), ref, 0.5 * ref ** 3 * TWO_M24 * D * (E2 + 2 * m.abs() * Ea) + 0.5 * ulp(ref, F32), f"{what}: rstd")
    c = torch.arange(C) >= 3
    err = ((rstd.values().double() - ref).abs() / (0.5 * ref ** 3 * TWO_M24 * D * (E2 + 2 * m.abs() * Ea) + 0.5 * ulp(ref, F32)))
    print(f"{what}: rstd uses {float(err[:, c].max()) if C > 3 else 0:.3f} of its bound on the well-conditioned channels, "
          f"{float(err[:, 1:3].max()):.4f} on the channels with mean / std = 100, 1000")
    if figures is not None:
        figures.append((what, a, b))
    return a, b


# ---- E: argument errors (HipBackend) ---------------------------------------------------------------------------------------------------
def run_argument_errors(be, dev):
    """Every entry point refuses C in 0, 16, 48, 96, 512 and rows_per_group = 0 with MMDYN_ERR_SHAPE before any launch (the guarded
    outputs keep the sentinel everywhere), and null pointers with MMDYN_ERR_NULL."""
    SHAPE, NULL = -1, -2
    lib = be.lib
    G, rpg, C0, T = 2, 40, 64, 2
    p = lambda x: None if x is None else x.data_ptr()
    x = torch.zeros(G * rpg * 512, device=dev)
    v = torch.ones(G * 512, device=dev)
    s64 = torch.zeros(G * 2 * 512, dtype=F64, device=dev)
    outs = [X.Guarded(G * rpg, 512, F32, dev) for _ in range(3)]
    o64 = X.Guarded(32 * G * 2, 512, F64, dev)
    opl = X.Guarded(G * rpg * 3, 512, BF16, dev)
    a, b, c = (p(o.t) for o in outs)

    def calls(C, r):
        return {
            "mmdyn_colstats": lambda: lib.mmdyn_colstats(p(x), a, G, r, C, None),
            "mmdyn_bn_finalize": lambda: lib.mmdyn_bn_finalize(p(x), a, b, None, None, None, p(o64.t), G, T, C, r, 1e-5, 0.1, 1, None, None),
            "mmdyn_bn_swish_fwd": lambda: lib.mmdyn_bn_swish_fwd(p(x), p(v), p(v), p(v), p(v), a, G, r, C, None),
            "mmdyn_bn_swish_bwd_reduce": lambda: lib.mmdyn_bn_swish_bwd_reduce(p(x), p(x), p(v), p(v), p(v), p(v), a, G, r, C, None),
            "mmdyn_bn_swish_bwd_apply": lambda: lib.mmdyn_bn_swish_bwd_apply(p(x), p(x), p(v), p(v), p(v), p(v), p(v), a, G, r, C, 0, None),
            "mmdyn_bn_swish_fwd_planes": lambda: lib.mmdyn_bn_swish_fwd_planes(p(x), p(v), p(v), p(v), p(v), a, p(opl.t), G, r, C, None),
            "mmdyn_bn_swish_bwd_apply_planes": lambda: lib.mmdyn_bn_swish_bwd_apply_planes(p(x), p(x), p(v), p(v), p(v), p(v), p(v), a, p(opl.t),
                                                                                          G, r, C, 0, None),
            "mmdyn_bn_eval_swish_bwd": lambda: lib.mmdyn_bn_eval_swish_bwd(p(x), p(x), p(v), p(v), p(v), p(v), a, p(opl.t), b, G, r, C, 0, None),
        }

    def calls_c(C):         # (no rows_per_group argument)
        return {
            "mmdyn_bn_reduce_partials": lambda: lib.mmdyn_bn_reduce_partials(p(x), p(o64.t), p(o64.t), G, T, C, None),
            "mmdyn_bn_finalize_sums": lambda: lib.mmdyn_bn_finalize_sums(p(s64), a, b, None, None, None, G, C, rpg, 1e-5, 0.1, 1, None),
            "mmdyn_bn_bwd_finalize": lambda: lib.mmdyn_bn_bwd_finalize(p(x), a, b, c, p(o64.t), G, T, C, 0.0, None, None),
            "mmdyn_bn_bwd_finalize_sums": lambda: lib.mmdyn_bn_bwd_finalize_sums(p(s64), a, b, c, G, C, 1.0, 0.0, None),
        }

    for C in (0, 16, 48, 96, 512):
        for name, call in {**calls(C, rpg), **calls_c(C)}.items():
            assert call() == SHAPE, f"{name} with C = {C} returned {call()}, not MMDYN_ERR_SHAPE"
    for name, call in calls(C0, 0).items():
        assert call() == SHAPE, f"{name} with rows_per_group = 0 returned {call()}, not MMDYN_ERR_SHAPE"
    assert lib.mmdyn_bn_eval_stats(p(v), p(v), a, b, G, 0, 1e-5, None) == SHAPE
    assert lib.mmdyn_bn_finalize(p(x), a, b, None, None, None, p(o64.t), G, 0, C0, rpg, 1e-5, 0.1, 1, None, None) == SHAPE
    assert lib.mmdyn_bn_finalize_sums(p(s64), a, b, None, None, None, G, C0, 0, 1e-5, 0.1, 1, None) == SHAPE
    null = {
        "mmdyn_colstats": [lambda: lib.mmdyn_colstats(None, a, G, rpg, C0, None), lambda: lib.mmdyn_colstats(p(x), None, G, rpg, C0, None)],
        "mmdyn_bn_finalize": [lambda: lib.mmdyn_bn_finalize(None, a, b, None, None, None, p(o64.t), G, T, C0, rpg, 1e-5, 0.1, 1, None, None),
                              lambda: lib.mmdyn_bn_finalize(p(x), None, b, None, None, None, p(o64.t), G, T, C0, rpg, 1e-5, 0.1, 1, None, None),
                              lambda: lib.mmdyn_bn_finalize(p(x), a, None, None, None, None, p(o64.t), G, T, C0, rpg, 1e-5, 0.1, 1, None, None),
                              lambda: lib.mmdyn_bn_finalize(p(x), a, b, None, None, None, None, G, T, C0, rpg, 1e-5, 0.1, 1, None, None)],
        "mmdyn_bn_swish_fwd": [lambda: lib.mmdyn_bn_swish_fwd(p(x), p(v), p(v), p(v), p(v), None, G, rpg, C0, None),
                               lambda: lib.mmdyn_bn_swish_fwd(None, p(v), p(v), p(v), p(v), a, G, rpg, C0, None),
                               lambda: lib.mmdyn_bn_swish_fwd(p(x), p(v), None, p(v), p(v), a, G, rpg, C0, None)],
        "mmdyn_bn_swish_bwd_reduce": [lambda: lib.mmdyn_bn_swish_bwd_reduce(p(x), p(x), p(v), p(v), p(v), p(v), None, G, rpg, C0, None),
                                      lambda: lib.mmdyn_bn_swish_bwd_reduce(None, p(x), p(v), p(v), p(v), p(v), a, G, rpg, C0, None)],
        "mmdyn_bn_swish_bwd_apply": [lambda: lib.mmdyn_bn_swish_bwd_apply(p(x), p(x), p(v), p(v), p(v), p(v), None, a, G, rpg, C0, 0, None),
                                     lambda: lib.mmdyn_bn_swish_bwd_apply(p(x), p(x), p(v), p(v), p(v), p(v), p(v), None, G, rpg, C0, 0, None)],
        "mmdyn_bn_swish_fwd_planes": [lambda: lib.mmdyn_bn_swish_fwd_planes(p(x), p(v), p(v), p(v), p(v), a, None, G, rpg, C0, None)],
        "mmdyn_bn_swish_bwd_apply_planes": [lambda: lib.mmdyn_bn_swish_bwd_apply_planes(p(x), p(x), p(v), p(v), p(v), p(v), p(v), a, None, G, rpg,
                                                                                       C0, 0, None)],
        "mmdyn_bn_eval_stats": [lambda: lib.mmdyn_bn_eval_stats(None, p(v), a, b, G, C0, 1e-5, None),
                                lambda: lib.mmdyn_bn_eval_stats(p(v), p(v), a, None, G, C0, 1e-5, None)],
        "mmdyn_bn_reduce_partials": [lambda: lib.mmdyn_bn_reduce_partials(p(x), None, p(o64.t), G, T, C0, None),
                                     lambda: lib.mmdyn_bn_reduce_partials(p(x), p(o64.t), None, G, T, C0, None)],
        "mmdyn_bn_finalize_sums": [lambda: lib.mmdyn_bn_finalize_sums(None, a, b, None, None, None, G, C0, rpg, 1e-5, 0.1, 1, None),
                                   lambda: lib.mmdyn_bn_finalize_sums(p(s64), a, None, None, None, None, G, C0, rpg, 1e-5, 0.1, 1, None)],
        "mmdyn_bn_bwd_finalize": [lambda: lib.mmdyn_bn_bwd_finalize(None, a, b, c, p(o64.t), G, T, C0, 0.0, None, None),
                                  lambda: lib.mmdyn_bn_bwd_finalize(p(x), None, b, c, p(o64.t), G, T, C0, 0.0, None, None),
                                  lambda: lib.mmdyn_bn_bwd_finalize(p(x), a, b, c, None, G, T, C0, 0.0, None, None)],
        "mmdyn_bn_bwd_finalize_sums": [lambda: lib.mmdyn_bn_bwd_finalize_sums(None, a, b, c, G, C0, 1.0, 0.0, None)],
        "mmdyn_act_fwd": [lambda: lib.mmdyn_act_fwd(None, a, 8, 1, None), lambda: lib.mmdyn_act_fwd(p(x), None, 8, 1, None)],
        "mmdyn_act_bwd": [lambda: lib.mmdyn_act_bwd(None, p(x), a, 8, 1, None), lambda: lib.mmdyn_act_bwd(p(x), None, a, 8, 1, None),
                          lambda: lib.mmdyn_act_bwd(p(x), p(x), None, 8, 1, None)],
    }
    for name, cs in null.items():
        for i, call in enumerate(cs):
            assert call() == NULL, f"{name}, null pointer case {i}: returned {call()}, not MMDYN_ERR_NULL"
    _sync(dev)
    for i, o in enumerate(outs + [o64, opl]):
        o.check(f"argument errors: output {i}")
        assert bool((bits(o.values()) == bits(o.buf[:1])[0]).all()), f"argument errors: output {i} was written by a refused call"


if __name__ == "__main__":
    measure()
