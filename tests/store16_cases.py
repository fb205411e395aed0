"""Per-element checks for results that pass through exp / rcp on their way into a 16-bit (or fp32) store: the BatchNorm + Swish
element-wise kernels of the storage modes and the Swish / BatchNorm-backward epilogues of the GEMMs.  Shared by
tests/test_store16_emu.py (CPU: the emulation and a plain torch-fp32 evaluation) and tests/test_store16_gpu.py (HipBackend).

Reference: the documented formula of the entry point (include/mmdyn_hip.h), evaluated in torch fp64 on exactly the widened 16-bit
inputs (`formulas` below with dtype = float64; it never goes through EmuBackend).  The GEMM epilogues run on the integer operands of
tests/exact_cases.py (family A), so the accumulator is exact and the epilogue is the only rounding.

Rule for an output tensor of storage type T (bf16, half, fp32), `check_rule`:
  1. every element: |got - ref| <= 1/2 ulp_T(ref) + c * 2^-24 * M, with M the largest intermediate magnitude of that element (the
     reference computes it per kernel, in fp64) and ulp_T the subnormal spacing below the smallest normal.  Beyond the largest
     finite value of T the store must give +-inf where |ref| - c 2^-24 M is past the rounding threshold (65520 for half), and may
     give it only where |ref| + c 2^-24 M reaches the threshold: RNE into subnormals and into +-inf, as torch's .to(T) gives.
  2. 16-bit T: at most max(2, 0.5 %) of the elements differ in bits from RNE_T(ref): round-to-nearest passes, truncation (about
     50 %) does not.  A condition, not a measurement.  (Not for T = fp32: an fp32 evaluation carries its own last-bit error, and
     the plain CPU one already differs from RNE_fp32(ref) in 40 to 53 % of the elements; rule 1 is the check there.)
  3. outputs sit in exact_cases.Guarded buffers; fp32 side outputs (partial sums) keep the tolerances of the norm-wise tests,
     against the fp64 reference.

The constants c are MEASURED, not guessed: c = 4 x the largest |r32 - ref| / (2^-24 M) of a plain torch-fp32 CPU evaluation of the
same formula (`formulas` with dtype = float32) over exactly the inputs below, both storage types; the factor 4 is for the device's
v_exp_f32 / v_rcp_f32 and its other operation order.  `measure()` prints them (python tests/store16_cases.py); test_store16_emu.py
asserts that the fp32 evaluation stays within a quarter of the bound, so a constant that no longer matches its inputs fails there.

A plain module, like tests/exact_cases.py; no fixture, no pytest setting.
"""
import math

import torch

import exact_cases as X
from dirty import bits
from mmdyn_hip.ops import CONV, TCONV_S2P1, TCONV_S1P0

F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
TWO_M24 = 2.0 ** -24
MANT = {BF16: 8, F16: 11, F32: 24}               # significand bits
E_MIN = {BF16: -126, F16: -14, F32: -126}        # exponent of the smallest normal
E_MAX = {BF16: 127, F16: 15, F32: 127}
CAP = 0.005                                      # rule 2

# c per kernel: 4 x the largest value of the fp32 evaluation over all shapes and both storage types, rounded up (the measured maximum
# in the comment; measure() prints the table).  With da_is_du = 0 the apply pass inherits the cancellation of swish' near its zero at
# u = -1.2785: there du -> 0 while its absolute error stays 2^-24 |da| sigmoid(u), and M, which counts |du| and the two mean terms
# only, gets small -- the measured maximum is one such element ((1, 1, 256), bf16: 155; 15 to 121 on the other shapes).
C_FWD = 18.0             # bn_swish_fwd: 4.49 (half, (3, 1000, 64); the scaled half inputs: 4.49)
C_APPLY = 622.0          # bn_swish_bwd_apply, da_is_du = 0: 155.35
C_APPLY_DU = 14.0        # bn_swish_bwd_apply, da_is_du = 1: 3.47
C_ACT_BWD = 15.0         # act_bwd (Swish): 3.68
C_SWISH_OUT = 9.0        # Swish second output of igemm_nt: 2.04
C_DGRAD_ACT = 20.0       # igemm_nt_dgrad_act (Swish): 4.84 (fp32 operands; 4.11 with 16-bit u)
C_DGRAD_BN = 32.0        # igemm_nt_dgrad_bn C: 7.85 (fp32 operands; 7.72 with 16-bit y)

BN_SHAPES = [(3, 1000, 64), (2, 129, 32), (1, 1, 256), (4, 63, 128)]          # G, rows per group, C
# mode, G, Bg, Hi, Cin, Ho, N, stride, offset: IGEMM_CASES[4], [6], [9], [13] of tests/test_kernels_gpu.py
EPI_CASES = [(CONV, 1, 4, 32, 32, 16, 64, 2, -1), (CONV, 1, 5, 8, 128, 5, 256, 1, 0), (TCONV_S2P1, 2, 3, 16, 64, 32, 32, 1, 0),
             (TCONV_S1P0, 4, 70, 5, 256, 8, 128, 1, 0)]
# the all-16 persistent route: the shapes of test_exact_gpu.test_igemm_all16_persistent
ALL16_CASES = [(CONV, 2, 3, 16, 64, 8, 128, 2, -1), (TCONV_S2P1, 2, 5, 8, 128, 16, 64, 1, 0), (TCONV_S1P0, 2, 70, 5, 256, 8, 128, 1, 0)]


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def ulp(ref, T):
    """Spacing of T at |ref| (fp64): 2^(e - p + 1), e clamped to the normal range (subnormal spacing below, top binade above)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -300))).clamp(E_MIN[T], E_MAX[T])
    # (log2 of a value just below a power of two may round up to it: settle the exponent by comparison)
    e = torch.where(torch.exp2(e) > ref.abs(), e - 1, e).clamp(E_MIN[T], E_MAX[T])
    return torch.exp2(e - (MANT[T] - 1))


def inf_threshold(T):
    """|x| >= this rounds to infinity under RNE: the largest finite value plus half its spacing."""
    return (2.0 - 2.0 ** -MANT[T]) * 2.0 ** E_MAX[T]


def rne(ref, T):
    """RNE_T(ref) as fp64 values (+-inf beyond the threshold), computed in fp64 integer arithmetic: no double rounding."""
    q = ulp(ref, T)
    r = torch.round(ref / q) * q                     # (torch.round: half to even; ref / q is exact, q a power of two)
    return torch.where(ref.abs() >= inf_threshold(T), torch.copysign(torch.full_like(ref, math.inf), ref), r)


def check_rule(got, ref, M, T, c, what, figures=None):
    """Rules 1 and 2 for one output [rows][columns] of type T against the fp64 reference and its magnitudes M.  A failure names
    the first offending element, its (row, column), both values and the bound.  -> (largest |err| / bound, share that differs in
    bits from RNE_T(ref)), also appended to `figures` and printed."""
    got = got.detach().cpu()
    assert got.dtype == T and got.shape == ref.shape == M.shape, (what, got.dtype, tuple(got.shape), tuple(ref.shape))
    assert ref.dtype == F64 and M.dtype == F64 and bool(torch.isfinite(ref).all()) and bool((M >= 0).all())
    g, cols = got.double().reshape(-1), got.shape[-1]
    ref, M = ref.reshape(-1), M.reshape(-1)
    slack = c * TWO_M24 * M
    bound = 0.5 * ulp(ref, T) + slack
    thr = inf_threshold(T)
    fin = torch.isfinite(g)
    err = torch.where(fin, (g - ref).abs(), torch.zeros_like(ref))
    bad = fin & ((err > bound) | (ref.abs() - slack >= thr))                                  # too far, or finite where inf is due
    bad |= torch.isinf(g) & ((ref.abs() + slack < thr) | (torch.sign(g) != torch.sign(ref)))  # inf where it is not due
    bad |= torch.isnan(g)
    ratio = float((err / bound).max())
    want = rne(ref, T).to(T)
    differ = bits(got) != bits(want.reshape(got.shape))
    share = float(differ.sum()) / differ.numel()
    line = f"{what}: largest |got - ref| / bound = {ratio:.3f}, {int(differ.sum())} of {differ.numel()} elements ({share:.2e}) differ from RNE"
    print(line)
    if figures is not None:
        figures.append((what, ratio, share))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements break rule 1, the first at flat index {i} (row {i // cols}, "
                             f"column {i % cols}): reference {ref[i].item()!r}, found {g[i].item()!r}, |difference| "
                             f"{abs(g[i].item() - ref[i].item())!r} against 1/2 ulp + c 2^-24 M = {bound[i].item()!r} (c = {c}, M = {M[i].item()!r})")
    allowed = max(2, int(CAP * differ.numel()))
    if T != F32 and int(differ.sum()) > allowed:
        i = int(differ.nonzero()[0])
        raise AssertionError(f"{what}: {int(differ.sum())} of {differ.numel()} elements differ in bits from the RNE-rounded reference "
                             f"(rule 2 allows {allowed}), the first at flat index {i} (row {i // cols}, column {i % cols}): expected "
                             f"{want.reshape(-1)[i].item()!r}, found {g[i].item()!r}")
    return ratio, share


def rel_l2(got, ref):
    return float((got.double() - ref).norm() / (ref.norm() + 1e-300))


# ---- the documented formulas, in one dtype (float64: the reference; float32: its plain CPU twin) -----------------------------------
def _sigmoid(v):
    return 1 / (1 + torch.exp(-v))


def swish(v):
    return v * _sigmoid(v)


def swish_grad(v):
    s = _sigmoid(v)
    return s * (1 + v * (1 - s))


def swish_grad_mag(v):
    """Largest intermediate of swish_grad: s * (1 + |v (1 - s)|)."""
    s = _sigmoid(v)
    return s * (1 + (v * (1 - s)).abs())


def _xhat(y, mean, rstd, G, rpg, C):
    return (y.reshape(G, rpg, C) - mean[:, None]) * rstd[:, None]


def f_fwd(dt, y, mean, rstd, gamma, beta, G, rpg, C):
    """a = swish(gamma * xhat + beta) -> (a, M = |gamma xhat| + |beta|), [G rpg][C]."""
    y, mean, rstd, gamma, beta = (t.to(dt) for t in (y, mean, rstd, gamma, beta))
    gx = gamma * _xhat(y, mean, rstd, G, rpg, C)
    return swish(gx + beta).reshape(-1, C), (gx.abs() + beta.abs()).expand(G, rpg, C).reshape(-1, C)


def f_du(dt, da, y, mean, rstd, gamma, beta, G, rpg, C):
    """(du = da * swish'(gamma xhat + beta), xhat), [G][rpg][C]."""
    da, y, mean, rstd, gamma, beta = (t.to(dt) for t in (da, y, mean, rstd, gamma, beta))
    xh = _xhat(y, mean, rstd, G, rpg, C)
    return da.reshape(G, rpg, C) * swish_grad(gamma * xh + beta), xh


def f_reduce(dt, da, y, mean, rstd, gamma, beta, G, rpg, C):
    """sums [G][2][C] = (sum du, sum du * xhat) over the rows of a group."""
    du, xh = f_du(dt, da, y, mean, rstd, gamma, beta, G, rpg, C)
    return torch.stack([du.sum(1), (du * xh).sum(1)], 1)


def f_apply(dt, da, y, mean, rstd, gamma, beta, sums, G, rpg, C, da_is_du):
    """dy = gamma rstd (du - s0 / n - xhat s1 / n) -> (dy, M = |gamma rstd| (|du| + |s0 / n| + |xhat s1 / n|))."""
    du, xh = f_du(dt, da, y, mean, rstd, gamma, beta, G, rpg, C)
    if da_is_du:
        du = da.to(dt).reshape(G, rpg, C)
    sums, gr = sums.to(dt), (gamma.to(dt) * rstd.to(dt))[:, None]
    t0, t1 = (sums[:, 0] / rpg)[:, None], xh * (sums[:, 1] / rpg)[:, None]
    return (gr * (du - t0 - t1)).reshape(-1, C), (gr.abs() * (du.abs() + t0.abs() + t1.abs())).reshape(-1, C)


def f_act_bwd(dt, dh, u):
    """du = dh * swish'(u) -> (du, M = |dh| * the largest intermediate of swish')."""
    dh, u = dh.to(dt), u.to(dt)
    return dh * swish_grad(u), dh.abs() * swish_grad_mag(u)


def f_swish_out(dt, v):
    """C_act = swish(v), v = acc + bias -> (C_act, M = |v|)."""
    v = v.to(dt)
    return swish(v), v.abs()


def f_dgrad_act(dt, acc, u):
    """C = acc * swish'(u) -> (C, M = |acc|)."""
    acc, u = acc.to(dt), u.to(dt)
    return acc * swish_grad(u), acc.abs()


def f_dgrad_bn(dt, acc, y, mean, rstd, gamma, beta, G, rpg, C):
    """C = du = acc * swish'(gamma xhat + beta), stats (sum du, sum du xhat) -> (C, M = |acc|, stats [G][2][C])."""
    du, xh = f_du(dt, acc, y, mean, rstd, gamma, beta, G, rpg, C)
    return du.reshape(-1, C), acc.to(dt).abs().reshape(-1, C), torch.stack([du.sum(1), (du * xh).sum(1)], 1)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _uniform(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


_BN = {}


def bn_inputs(shape, T, scaled=False):
    """y, da [G rpg][C] of type T and fp32 mean / rstd [G][C], gamma / beta [C] in the data range of the norm-wise tests
    (tests/test_kernels_gpu.py::test_elementwise_bf16_storage), built once per (shape, T).  scaled (half): gamma and beta of every
    fourth channel times 2^-17 (outputs below the smallest normal, 2^-14) and of every fourth times 2^16 (outputs to 7e5)."""
    key = (shape, T, scaled)
    if key not in _BN:
        G, rpg, C = shape
        g = torch.Generator().manual_seed(5100 + G * 1000003 + rpg * 1009 + C)
        y, da = (_uniform(g, G * rpg, C) * 2 + 0.3).to(T), _uniform(g, G * rpg, C).to(T)
        mean, rstd = _uniform(g, G, C) * 0.2, _uniform(g, G, C).abs() + 0.6
        gamma, beta = _uniform(g, C) + 1.5, _uniform(g, C)
        if scaled:
            k = torch.arange(C) % 4
            scale = torch.where(k == 1, 2.0 ** -17, torch.where(k == 3, 2.0 ** 16, 1.0))
            gamma, beta = gamma * scale, beta * scale
        _BN[key] = (y, da, mean, rstd, gamma, beta)
    return _BN[key]


_EPI = {}


def epi_inputs(case, T):
    """Integer operands of one GEMM case (thinned {-1, 0, 1}: accumulators of a few units, where the sigmoid is not flat) and the
    epilogue operands: bias in 64ths (acc + bias is exact in fp32, and rounds in bf16 from |v| = 2, in half from 16 on), u / y of the storage type, BatchNorm parameters.
    -> dict, built once per (case, T); T None: fp32 everywhere."""
    key = (tuple(case), T)
    if key not in _EPI:
        g = X.Geo(case)
        A, Bp = X.int_operands(g, 611, sparse=True)
        acc = X.assert_int_exact(g, A, Bp, out16=T)
        gen = torch.Generator().manual_seed(6100 + g.rows + 7 * g.N)
        bias = X.ints((g.N,), 613, 64) / 64
        cast = (lambda t: t.to(T)) if T else (lambda t: t)
        u = cast(_uniform(gen, g.rows, g.N) * 3)
        y = cast(_uniform(gen, g.rows, g.N) * 1.5 + 0.2)
        mean, rstd = _uniform(gen, g.G, g.N) * 0.3, _uniform(gen, g.G, g.N).abs() + 0.5
        gamma, beta = _uniform(gen, g.N) + 1.2, _uniform(gen, g.N)
        _EPI[key] = dict(g=g, A=A, Bp=Bp, acc=acc, bias=bias, u=u, y=y, mean=mean, rstd=rstd, gamma=gamma, beta=beta)
    return _EPI[key]


# ---- runners: element-wise kernels -----------------------------------------------------------------------------------------------
def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def run_fwd(be, dev, shape, T, scaled=False, figures=None, what="", inputs=None, c=C_FWD):
    """mmdyn_bn_swish_fwd_b16 (T = fp32: mmdyn_bn_swish_fwd).  scaled: part of the output is subnormal in half and part lies beyond
    65504.  inputs / c: another input set (y, da, mean, rstd, gamma, beta) with the constant measured on it (tests/bn_cases.py)."""
    G, rpg, C = shape
    y, _, mean, rstd, gamma, beta = inputs or bn_inputs(shape, T, scaled)
    ref, M = f_fwd(F64, y, mean, rstd, gamma, beta, G, rpg, C)
    if scaled:      # (preconditions, on the reference alone)
        tiny, huge = (ref.abs() < 2.0 ** E_MIN[T]) & (ref.abs() > 2.0 ** (E_MIN[T] - MANT[T] + 2)), ref.abs() > 1.01 * inf_threshold(T)
        assert int(tiny.sum()) >= ref.numel() // 16 and int(huge.sum()) >= ref.numel() // 64 and int((~huge).sum()) >= ref.numel() // 2
    a = X.Guarded(G * rpg, C, T, dev)
    be.bn_swish_fwd(y.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), beta.to(dev), a.view(G * rpg, C), G, rpg, C)
    _sync(dev)
    what = f"{what}bn_swish_fwd {shape} {T}{' scaled' if scaled else ''}"
    a.check(what)
    return check_rule(a.values(), ref, M, T, c, what, figures)


def reduce_ref(shape, T):
    y, da, mean, rstd, gamma, beta = bn_inputs(shape, T)
    return f_reduce(F64, da, y, mean, rstd, gamma, beta, *shape)


def run_reduce(be, dev, shape, T, figures=None, what=""):
    """mmdyn_bn_swish_bwd_reduce_b16: the [G][T][2][C] partials summed over the tiles against fp64 sums, at the tolerance of the
    norm-wise test (relative L2 1e-4)."""
    G, rpg, C = shape
    y, da, mean, rstd, gamma, beta = bn_inputs(shape, T)
    tiles = be.colstats_tiles(rpg)
    P = X.Guarded(G * tiles * 2, C, F32, dev)
    be.bn_swish_bwd_reduce(da.to(dev), y.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), beta.to(dev), P.view(G, tiles, 2, C),
                           G, rpg, C)
    _sync(dev)
    what = f"{what}bn_swish_bwd_reduce {shape} {T}"
    P.check(what)
    got, ref = P.values().double().reshape(G, tiles, 2, C).sum(1), reduce_ref(shape, T)
    r = rel_l2(got, ref)
    print(f"{what}: relative L2 of the partial sums against fp64 = {r:.3e}")
    if figures is not None:
        figures.append((what, r, None))
    assert r <= 1e-4, f"{what}: partial sums differ from the fp64 sums by relative L2 {r:.3e} > 1e-4"
    return r


def run_apply(be, dev, shape, T, da_is_du, figures=None, what="", inputs=None, c=None):
    """mmdyn_bn_swish_bwd_apply_b16 (T = fp32: mmdyn_bn_swish_bwd_apply); the sums are the fp64 sums of the reduce pass, rounded to
    fp32.  inputs / c: as in run_fwd."""
    G, rpg, C = shape
    y, da, mean, rstd, gamma, beta = inputs or bn_inputs(shape, T)
    sums = f_reduce(F64, da, y, mean, rstd, gamma, beta, *shape).float()
    ref, M = f_apply(F64, da, y, mean, rstd, gamma, beta, sums, G, rpg, C, da_is_du)
    dy = X.Guarded(G * rpg, C, T, dev)
    be.bn_swish_bwd_apply(da.to(dev), y.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), beta.to(dev), sums.to(dev),
                          dy.view(G * rpg, C), G, rpg, C, da_is_du)
    _sync(dev)
    what = f"{what}bn_swish_bwd_apply {shape} {T} da_is_du={int(da_is_du)}"
    dy.check(what)
    return check_rule(dy.values(), ref, M, T, c if c is not None else (C_APPLY_DU if da_is_du else C_APPLY), what, figures)


def run_act_bwd(be, dev, shape, T, act, figures=None, what="", inputs=None, c=C_ACT_BWD):
    """mmdyn_act_bwd_b16 (T = fp32: mmdyn_act_bwd): Swish by the rule; ReLU with `==` (du = dh where u > 0, zero elsewhere).
    inputs / c: another (u, dh) [G rpg][C] with the constant measured on it."""
    G, rpg, C = shape
    u, dh = inputs or bn_inputs(shape, T)[:2]
    du = X.Guarded(G * rpg, C, T, dev)
    be.act_bwd(dh.to(dev), u.to(dev), du.view(G * rpg, C), act)
    _sync(dev)
    what = f"{what}act_bwd {shape} {T} act={act}"
    du.check(what)
    if act == 2:
        assert bool((u.float() <= 0).any()) and bool((u.float() > 0).any())
        return X.check_exact(du.values(), dh.double() * (u.double() > 0), what)
    ref, M = f_act_bwd(F64, dh, u)
    return check_rule(du.values(), ref, M, T, c, what, figures)


# ---- runners: GEMM epilogues -----------------------------------------------------------------------------------------------------
def _operands(e, T, all16, dev):
    A, Bp = e["A"], e["Bp"]
    return (A.to(T) if T else A).to(dev), (Bp.to(T) if all16 else Bp).to(dev)


def run_swish_out(be, dev, case, T, mixed=False, all16=False, figures=None, what=""):
    """mmdyn_igemm_nt with the Swish second output.  T: the storage type of A, C and C_act (None: fp32 everywhere); mixed: C stays
    fp32, C_act alone is 16-bit.  C = acc + bias is exact in fp32 (bias in 64ths): a 16-bit C is compared bit for bit with the
    RNE-rounded value, an fp32 C with `==`; C_act by the rule."""
    e = epi_inputs(case, T)
    g, Tc = e["g"], T or F32
    v = e["acc"] + e["bias"].double()
    assert bool((v.float().double() == v).all())
    a, b = _operands(e, T, all16, dev)
    C = X.Guarded(g.rows, g.N, F32 if mixed else Tc, dev)
    Ca = X.Guarded(g.rows, g.N, Tc, dev)
    be.igemm_nt(a, b, e["bias"].to(dev), C.t, Ca.t, None, None, *g.dims, g.N, g.stride, g.offset, 1, 1)
    _sync(dev)
    what = f"{what}igemm_nt Swish output {case} {T}{' mixed' if mixed else ''}{' all16' if all16 else ''}"
    C.check(f"{what}: C")
    Ca.check(f"{what}: C_act")
    X.check_exact(C.values(), rne(v, C.buf.dtype), f"{what}: C", bitwise=True)
    ref, M = f_swish_out(F64, v)
    return check_rule(Ca.values(), ref, M, Tc, C_SWISH_OUT, f"{what}: C_act", figures)


def run_dgrad_act(be, dev, case, T, all16=False, figures=None, what=""):
    """mmdyn_igemm_nt_dgrad_act with Swish: C = acc * swish'(u); A, u and C of type T (None: fp32)."""
    e = epi_inputs(case, T)
    g, Tc = e["g"], T or F32
    a, b = _operands(e, T, all16, dev)
    C = X.Guarded(g.rows, g.N, Tc, dev)
    be.igemm_nt_dgrad_act(a, b, C.t, e["u"].to(dev), 1, *g.dims, g.stride, g.offset)
    _sync(dev)
    what = f"{what}igemm_nt_dgrad_act Swish {case} {T}{' all16' if all16 else ''}"
    C.check(what)
    ref, M = f_dgrad_act(F64, e["acc"], e["u"])
    return check_rule(C.values(), ref, M, Tc, C_DGRAD_ACT, what, figures)


def run_dgrad_bn(be, dev, case, T, all16=False, figures=None, what=""):
    """mmdyn_igemm_nt_dgrad_bn: C = du by the rule; the per-tile (sum du, sum du xhat), summed over the tiles, against fp64 sums at
    the tolerances of the norm-wise tests (relative L2 5e-5 in fp32, 4e-3 with 16-bit storage)."""
    e = epi_inputs(case, T)
    g, Tc = e["g"], T or F32
    rpg = g.rows // g.G
    a, b = _operands(e, T, all16, dev)
    tiles = be.igemm_stat_tiles(*g.dims, **({"all16": True} if all16 else {}))
    C = X.Guarded(g.rows, g.N, Tc, dev)
    st = X.Guarded(g.G * tiles * 2, g.N, F32, dev)
    be.igemm_nt_dgrad_bn(a, b, C.t, st.view(g.G, tiles, 2, g.N), e["y"].to(dev), e["mean"].to(dev), e["rstd"].to(dev),
                         e["gamma"].to(dev), e["beta"].to(dev), *g.dims, g.stride, g.offset)
    _sync(dev)
    what = f"{what}igemm_nt_dgrad_bn {case} {T}{' all16' if all16 else ''}"
    C.check(f"{what}: C")
    st.check(f"{what}: stats")
    ref, M, sums = f_dgrad_bn(F64, e["acc"], e["y"], e["mean"], e["rstd"], e["gamma"], e["beta"], g.G, rpg, g.N)
    r = rel_l2(st.values().double().reshape(g.G, tiles, 2, g.N).sum(1), sums)
    tol = 4e-3 if T else 5e-5
    print(f"{what}: relative L2 of the stats against fp64 = {r:.3e}")
    if figures is not None:
        figures.append((f"{what}: stats", r, None))
    assert r <= tol, f"{what}: stats differ from the fp64 sums by relative L2 {r:.3e} > {tol}"
    return check_rule(C.values(), ref, M, Tc, C_DGRAD_BN, f"{what}: C", figures)


# ---- the fp32 twin: how the constants were measured, and that the cap of rule 2 is reachable -------------------------------------
def twins(T):
    """(name, c, r32, ref, M) of a plain torch-fp32 evaluation of every formula over the inputs above, storage type T (None: the
    fp32 epilogues)."""
    out = []
    if T is not None:
        for shape in BN_SHAPES:
            for scaled in ((False, True) if T == F16 else (False,)):
                y, da, mean, rstd, gamma, beta = bn_inputs(shape, T, scaled)
                out.append((f"fwd {shape}{' scaled' if scaled else ''}", C_FWD, f_fwd(F32, y, mean, rstd, gamma, beta, *shape)[0],
                            *f_fwd(F64, y, mean, rstd, gamma, beta, *shape)))
            y, da, mean, rstd, gamma, beta = bn_inputs(shape, T)
            sums = reduce_ref(shape, T).float()
            for is_du in (False, True):
                out.append((f"apply {shape} da_is_du={int(is_du)}", C_APPLY_DU if is_du else C_APPLY, f_apply(F32, da, y, mean, rstd, gamma, beta, sums, *shape, is_du)[0],
                            *f_apply(F64, da, y, mean, rstd, gamma, beta, sums, *shape, is_du)))
            out.append((f"act_bwd {shape}", C_ACT_BWD, f_act_bwd(F32, da, y)[0], *f_act_bwd(F64, da, y)))
    for case in EPI_CASES:
        e = epi_inputs(case, T)
        g = e["g"]
        v = e["acc"] + e["bias"].double()
        out.append((f"swish_out {case}", C_SWISH_OUT, f_swish_out(F32, v)[0], *f_swish_out(F64, v)))
        out.append((f"dgrad_act {case}", C_DGRAD_ACT, f_dgrad_act(F32, e["acc"], e["u"])[0], *f_dgrad_act(F64, e["acc"], e["u"])))
        bn = (e["acc"], e["y"], e["mean"], e["rstd"], e["gamma"], e["beta"], g.G, g.rows // g.G, g.N)
        out.append((f"dgrad_bn {case}", C_DGRAD_BN, f_dgrad_bn(F32, *bn)[0], *f_dgrad_bn(F64, *bn)[:2]))
    return out


def twin_figures(T):
    """[(name, c, largest |r32 - ref| / (2^-24 M), share of the T-rounded r32 that differs in bits from RNE_T(ref))]."""
    rows = []
    for name, c, r32, ref, M in twins(T):
        ok = M > 0
        ratio = float(((r32.double() - ref).abs()[ok] / (TWO_M24 * M[ok])).max())
        Tc = T or F32
        share = float((bits(r32.to(Tc)) != bits(rne(ref, Tc).to(Tc))).sum()) / ref.numel()
        rows.append((name, c, ratio, share))
    return rows


def measure():
    for T in (BF16, F16, None):
        for name, c, ratio, share in twin_figures(T):
            print(f"{str(T):16s} {name:70s} c = {c:5.1f}  measured {ratio:6.2f}  differs from RNE {share:.2e}")


if __name__ == "__main__":
    measure()
