"""Per-element checks for the fused last decoder layer: mmdyn_tconv_out3_bn_fwd, _bn_bce, _bn_bce_rows, _bn_bce_rows_grad
(csrc/tconv_out3.hip: the FUSED / LOSS / ROWS / Out3LossW instances of tconv_out3_kernel) and mmdyn_wgrad_out3_bn (csrc/conv3.hip:
conv3_wgrad_kernel<..., BNACT = true>).  Shared by tests/test_out3_emu.py (EmuBackend and a plain torch-fp32 evaluation, CPU) and
tests/test_out3_gpu.py (HipBackend).

References: the documented formulas of include/mmdyn_hip.h in torch fp64 on exactly the values the kernel reads (a 16-bit y is
widened first); they never go through EmuBackend.

Inputs: y fp32 / bf16 / half; mean, rstd per (group, channel), gamma, beta per channel; gamma in two sign patterns (channel c is
positive where (c + p) is even, p = 0 / 1), beta of both signs; every fifth channel has |gamma| of 11 to 12, so that u = gamma
xhat + beta covers about +-30 there (beyond +-24 on every shape, beyond +-30 on some), the others stay within +-3.  With the +-2^k
selection weights, |k| <= 3, the logits reach from about -120 to +240 over the shapes, and below -75 and above +175 on every one
(the largest scales the six sets put on the wide channels are -4 and +8): both branches of bce_elem; exp(-|x|) underflows on
every shape; sigmoid - t is -t or 1 - t to the last bit at both ends.  test_out3_emu.py asserts these figures.  Targets in [0, 1]
with exact 0 and 1, masks 0 / 1 with 1 and 3 channels, w_rec (0.37, 0, 1) per sample.

Selection family (every entry point): W one-hot per output channel, +-2^k, the six sets of exact_cases.out3_weight_sets: a logit is
scale * swish(u) of ONE input element or exactly 0 where the tap falls into the padding; the weight gradient of a one-hot Gt
likewise.  Rule: store16_cases.check_rule with T = fp32, M = |scale| (|gamma xhat| + |beta|), every element; padding `== 0`.
Dense family: small arbitrary fp32 W against fp64 ATen, M the same convolution of (|gamma xhat| + |beta|) with |W|.
Loss epilogue: dlogit per element,
    |got - ref| <= 1/2 ulp(ref) + |grad_scale w mk| (1/4 |mk| bound_x + C_D 2^-24 (sigmoid + |t mk|)),
bound_x the logit's own bound (|d sigmoid / dx| <= 1/4); exact zeros for discarded groups and masked-out elements; published
logits bit-identical to mmdyn_tconv_out3_bn_fwd's; loss tables per ENTRY on pre-filled tables (2e-6 relative of the fp64 sum, the
tolerance of the norm-wise tests; entries not addressed keep their bits; rows sum to the batch launch's slot to 1e-12).
Every output sits in an exact_cases.Guarded buffer (the fp64 tables too), every band is checked after every launch.

The constants C are MEASURED by the protocol of store16_cases.py: 4 x the largest |r32 - ref| / (2^-24 M) of a plain torch-fp32 CPU
evaluation of the same formula over exactly these inputs (`measure()` prints the table: python tests/out3_cases.py);
test_out3_emu.py asserts that the fp32 evaluation stays within a quarter of each bound.  Elements whose reference lies below the
smallest fp32 normal (a gradient whose sigmoid underflows: exp(89) is already infinite in fp32) are left out of the MEASUREMENT
of C_D, and of that constant alone: 2^-24 M is no measure where fp32 has no relative precision; the CHECK covers them, through
the logit's own bound.
The GPU's own error never sets a constant.

A plain module, like tests/exact_cases.py; no fixture, no pytest setting.
"""
import torch
import torch.nn.functional as F

import exact_cases as X
from dirty import bits
from mmdyn_hip._lib import MmdynError
from mmdyn_hip.ops import IM2COL3, TCONV_S2P1
from store16_cases import BF16, F16, F32, F64, TWO_M24, check_rule, f_fwd, ulp

# 4 x the measured maximum of the fp32 evaluation, rounded up (measure(); docs/LAB_NOTES.md has the table)
C_ACT = 20.0             # swish(gamma xhat + beta), selection logits and one-hot weight gradients: 4.89 (bf16, (2, 2, 32, 32), pattern 1)
C_DENSE = 18.0           # dense logits: 4.38 (half, (2, 3, 32, 32), pattern 1) -- the activation's error and the sum over 128 terms
C_D = 14.0               # dlogit on an exactly given logit: 3.35 (fp32, (1, 1, 48, 48))
C_W = 7.0                # dense weight gradient: 1.65 (bf16, (1, 1, 128), pattern 0)

TYPES = {"fp32": F32, "bf16s": BF16, "fp16s": F16}
# G, Bg, Hi, Wi: single tile (every halo cell is padding) / tile boundary in x only / in y only / three tiles in y / boundaries in
# both directions / one interior tile
FWD_SHAPES = [(1, 1, 16, 16), (2, 2, 16, 32), (3, 1, 32, 16), (1, 2, 48, 16), (2, 3, 32, 32), (1, 1, 48, 48)]
SLOTS_SHAPE = (4, 2, 16, 16)            # slots [5, -1, 0, 0]: a discarded group and two groups that share a slot
LOSS_SHAPES = FWD_SHAPES + [SLOTS_SHAPE]
WGRAD_SHAPES = [(2, 2, 32), (3, 1, 64), (1, 1, 128)]        # G, Bg, Hr: the sizes mmdyn_conv3_wgrad_try serves
WGRAD_REFUSED = [16, 48, 96, 256]                           # ... and sizes it does not (MMDYN_ERR_SHAPE before any launch)
N_SLOTS = 8
GRAD_SCALE = 0.37
W_REC = [0.37, 0.0, 1.0]
# TABLE_TOL: an addressed entry against the fp64 sum; SAME_TOL: the rows of a slot against the batch launch's slot, relative to the
# latter and with nothing added (an entry nobody addresses gives 0 against 0; `got - initial` of tables that hold 1e3 to 1e5 costs
# an fp64 ulp per entry, 1e-11 at the most, against SAME_TOL |b| >= 2e-9)
TABLE_TOL, SAME_TOL = 2e-6, 1e-12
ENTRIES = ("bce", "rows", "rows_grad")
SETS = X.out3_weight_sets()
DENSE_W = (torch.rand(32, 3, 4, 4, generator=torch.Generator().manual_seed(7045)) * 2 - 1) * 0.2


def slots_of(G):
    return [5, -1, 0, 0] if G == 4 else ([5, -1, 0][:G] if G > 1 else [1])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
class Inputs:
    pass


_IN = {}


def inputs(shape, T):
    """Built once per (shape, T) and left unchanged; shape (G, Bg, Hi, Wi)."""
    key = (tuple(shape), T)
    if key not in _IN:
        G, Bg, Hi, Wi = shape
        g = torch.Generator().manual_seed(7100 + G * 1000003 + Bg * 10007 + Hi * 101 + Wi)
        u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
        i = Inputs()
        i.shape = tuple(shape)
        i.y = (u(G * Bg * Hi * Wi, 32) * 2 + 0.3).to(T)
        grp = torch.arange(G, dtype=F32)[:, None]
        i.mean, i.rstd = u(G, 32) * 0.2 + 0.05 * grp, 0.6 + 0.5 * torch.rand(G, 32, generator=g) + 0.05 * grp
        i.mag = torch.where(torch.arange(32) % 5 == 0, 12.0, 0.7) * (0.9 + 0.1 * torch.rand(32, generator=g))
        i.beta = u(32) * 0.5
        r = torch.rand(Bg, 3, 2 * Hi, 2 * Wi, generator=g)
        i.target = torch.where(r < 0.1, 0.0, torch.where(r > 0.9, 1.0, torch.rand(Bg, 3, 2 * Hi, 2 * Wi, generator=g)))
        i.masks = {c: (torch.rand(Bg, c, 2 * Hi, 2 * Wi, generator=g) > 0.3).float() for c in (1, 3)}
        i.w_rec = torch.tensor(W_REC[:Bg])
        _IN[key] = i
    return _IN[key]


def gamma_of(i, p):
    return torch.where((torch.arange(32) + p) % 2 == 0, 1.0, -1.0) * i.mag


def act_ref(dt, i, p):
    """(a, M) [rows][32] in dtype dt: a = swish(gamma xhat + beta), M = |gamma xhat| + |beta|."""
    G, Bg, Hi, Wi = i.shape
    return f_fwd(dt, i.y, i.mean, i.rstd, gamma_of(i, p), i.beta, G, Bg * Hi * Wi, 32)


_IDX = {}


def select_index(shape, s):
    """[Bt][3][Ho][Wo] long: 1 + the flat index into [rows][32] of the element weight set s selects, 0 where its tap falls into the
    padding -- exact_cases.select_ref on an activation that holds its own indices."""
    key = (tuple(shape), s)
    if key not in _IDX:
        G, Bg, Hi, Wi = shape
        Bt = G * Bg
        geo = X.Geo((TCONV_S2P1, 1, Bt, Hi, Wi, 32, 2 * Hi, 2 * Wi, 3, 1, 0))
        n = Bt * Hi * Wi * 32
        assert n < 1 << 24
        _, tap, ci, _ = SETS[s]
        idx = X.select_ref(geo, (torch.arange(n, dtype=F32) + 1).reshape(-1, 32), tap, ci, torch.ones(3))
        _IDX[key] = idx.long().reshape(Bt, 2 * Hi, 2 * Wi, 3).permute(0, 3, 1, 2).contiguous()
    return _IDX[key]


def select_logits(a, M, shape, s):
    """(logits, M, valid) [Bt][3][Ho][Wo] of the activation a [rows][32] (any dtype) under weight set s."""
    idx = select_index(shape, s)
    valid = idx > 0
    scale = SETS[s][3].to(a.dtype).reshape(1, 3, 1, 1)
    pick = lambda t: torch.where(valid, t.reshape(-1)[(idx - 1).clamp_min(0)], torch.zeros((), dtype=t.dtype))
    return pick(a) * scale, pick(M) * scale.abs(), valid


def dense_logits(a, M, shape, dt):
    G, Bg, Hi, Wi = shape
    nchw = lambda t: t.to(dt).reshape(G * Bg, Hi, Wi, 32).permute(0, 3, 1, 2)
    return (F.conv_transpose2d(nchw(a), DENSE_W.to(dt), stride=2, padding=1),
            F.conv_transpose2d(nchw(M), DENSE_W.abs().to(dt), stride=2, padding=1))


def logit_bound(ref, M):
    return 0.5 * ulp(ref, F32) + C_ACT * TWO_M24 * M


def loss_ref(dt, x, i, mask_c, slots, w_rec, bound_x=None):
    """The loss epilogue on logits x [Bt][3][Ho][Wo] in dtype dt -> dict: d (dlogit), Md (its magnitude |grad_scale w mk| (sigmoid +
    |t mk|)), extra (the share of the bound that comes from the logit's own), zero (elements that must be exactly zero), rows /
    rows_u [G][Bg] (sums per group and sample, masked / plain).  Target, mask and weight belong to the SAMPLE b mod Bg."""
    G, Bg, Hi, Wi = i.shape
    xg = x.to(dt).reshape(G, Bg, 3, 2 * Hi, 2 * Wi)
    t = i.target.to(dt)[None]
    mk = torch.ones((), dtype=dt) if not mask_c else i.masks[mask_c].to(dt).expand(Bg, 3, 2 * Hi, 2 * Wi)[None]
    live = torch.tensor([s >= 0 for s in slots]).reshape(G, 1, 1, 1, 1)
    xm, tm = xg * mk, (t * mk).expand_as(xg)
    sig = 1 / (1 + torch.exp(-xm))
    coef = (mk * torch.tensor(GRAD_SCALE, dtype=dt)) * w_rec.to(dt).reshape(1, Bg, 1, 1, 1) * live
    r = {"d": ((mk * (sig - tm) * torch.tensor(GRAD_SCALE, dtype=dt)) * w_rec.to(dt).reshape(1, Bg, 1, 1, 1) * live).reshape(x.shape),
         "Md": (coef.abs() * (sig + tm.abs())).reshape(x.shape),
         "zero": (~live | (mk.expand_as(xg) == 0)).reshape(x.shape)}
    if bound_x is not None:
        r["extra"] = (coef.abs() * 0.25 * mk.abs() * bound_x.reshape(xg.shape)).reshape(x.shape)
    r["rows"] = F.binary_cross_entropy_with_logits(xm, tm, reduction="none").sum((2, 3, 4))
    r["rows_u"] = F.binary_cross_entropy_with_logits(xg, t.expand_as(xg), reduction="none").sum((2, 3, 4))
    return r


def table_ref(rows, slots, per_sample):
    """(want [N_SLOTS][Bg or 1] fp64, addressed bool) of the sums rows [G][Bg]."""
    Bg = rows.shape[1]
    want = torch.zeros(N_SLOTS, Bg if per_sample else 1, dtype=F64)
    hit = torch.zeros_like(want, dtype=torch.bool)
    for g, s in enumerate(slots):
        if s >= 0:
            want[s] += rows[g].double() if per_sample else rows[g].double().sum()
            hit[s] = True
    return want, hit


# ---- launches --------------------------------------------------------------------------------------------------------------------
def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _args(i, p, w, dev):
    return tuple(t.to(dev) for t in (i.y, i.mean, i.rstd, gamma_of(i, p), i.beta, w))


def table_init(n):
    return 1000.125 + 3.25 * torch.arange(n, dtype=F64)


class Launch:
    """One launch of an entry point with every output in a Guarded buffer; `check()` looks at every band."""

    def __init__(self, be, dev, entry, i, p, w, lgroup=None, mask_c=0, slots=None, w_rec=None, want_dl=True, mask=None, what=""):
        G, Bg, Hi, Wi = i.shape
        Bt, Ho, Wo = G * Bg, 2 * Hi, 2 * Wi
        self.what, self.i, self.entry = what, i, entry
        slots = slots_of(G) if slots is None else slots
        args = _args(i, p, w, dev)
        self.out = self.dl = self.loss = self.unm = None
        if entry == "fwd":
            self.out = X.Guarded(Bt * 3 * Ho, Wo, F32, dev)
            be.tconv_out3_bn_fwd(*args, self.out.t, G, Bg, Hi, Wi)
            self.nb = Bt
        else:
            self.nb = Bt if lgroup is not None and lgroup < 0 else Bg
            if lgroup is not None:
                self.out = X.Guarded(self.nb * 3 * Ho, Wo, F32, dev)
            if entry == "rows_grad" or (entry == "bce" and want_dl):
                self.dl = X.Guarded(Bt * 3 * Ho, Wo, F32, dev)
            width = 1 if entry == "bce" else Bg
            self.loss, self.unm = X.Guarded(N_SLOTS, width, F64, dev), X.Guarded(N_SLOTS, width, F64, dev)
            self.init = table_init(N_SLOTS * width).reshape(N_SLOTS, width)
            for tab in (self.loss, self.unm):
                tab.t.copy_(self.init.reshape(-1))
            mask = (i.masks[mask_c] if mask_c else None) if mask is None else mask
            kw = dict(mask=None if mask is None else mask.to(dev), mask_channels=max(mask_c, 1))
            o, lg, tgt = None if self.out is None else self.out.t, -1 if lgroup is None else lgroup, i.target.to(dev)
            d = None if self.dl is None else self.dl.t
            if entry == "bce":
                be.tconv_out3_bn_bce(*args, o, lg, tgt, d, self.loss.view(N_SLOTS), slots, GRAD_SCALE, G, Bg, Hi, Wi,
                                     unmasked_slots=self.unm.view(N_SLOTS), **kw)
            elif entry == "rows":
                be.tconv_out3_bn_bce_rows(*args, o, lg, tgt, self.loss.view(N_SLOTS, Bg), slots, G, Bg, Hi, Wi,
                                          unmasked_rows=self.unm.view(N_SLOTS, Bg), **kw)
            else:
                wr = (i.w_rec if w_rec is None else w_rec).to(dev)
                be.tconv_out3_bn_bce_rows_grad(*args, o, lg, tgt, d, wr, self.loss.view(N_SLOTS, Bg), slots, GRAD_SCALE, G, Bg, Hi, Wi,
                                               unmasked_rows=self.unm.view(N_SLOTS, Bg), **kw)
        _sync(dev)
        for o, name in ((self.out, "logits"), (self.dl, "dlogit"), (self.loss, "loss table"), (self.unm, "unmasked table")):
            if o is not None:
                o.check(f"{what}: {name}")

    def logits(self):
        G, Bg, Hi, Wi = self.i.shape
        return self.out.values().reshape(self.nb, 3, 2 * Hi, 2 * Wi)

    def dlogit(self):
        G, Bg, Hi, Wi = self.i.shape
        return self.dl.values().reshape(G * Bg, 3, 2 * Hi, 2 * Wi)

    def delta(self, tab):
        return tab.values() - self.init


# ---- checks ----------------------------------------------------------------------------------------------------------------------
def _where(flat, shape):
    idx = []
    for n in reversed(shape):
        idx.append(flat % n)
        flat //= n
    return tuple(reversed(idx))


def check_zero(got, must, what):
    """got == 0 wherever `must`; names the first element (sample, channel, y, x) that is not."""
    bad = ((got != 0) | torch.isnan(got)) & must
    if bool(bad.any()):
        k = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(must.sum())} elements that must be exactly zero are not, the first at "
                             f"(sample, channel, y, x) = {_where(k, got.shape)}: found {got.reshape(-1)[k].item()!r}")


def check_logits(got, ref, M, valid, c, what, figures=None):
    """Rule 1 on every element ([Bt][3][Ho][Wo], rows (sample, channel, y)); valid given: the padding elements `== 0`."""
    Wo = got.shape[-1]
    r = check_rule(got.reshape(-1, Wo), ref.reshape(-1, Wo), M.reshape(-1, Wo), F32, c, what, figures)
    if valid is not None:
        check_zero(got, ~valid, f"{what}: taps in the padding")
    return r


def check_dlogit(got, lr, what, figures=None):
    """The per-element bound of dlogit (c = 1 on a magnitude that holds the whole slack) and the exact zeros."""
    Wo = got.shape[-1]
    Mall = (lr["extra"] + C_D * TWO_M24 * lr["Md"]) / TWO_M24
    r = check_rule(got.reshape(-1, Wo), lr["d"].reshape(-1, Wo), Mall.reshape(-1, Wo), F32, 1.0, what, figures)
    check_zero(got, lr["zero"], f"{what}: discarded groups and masked-out elements")
    return r


def check_table(tab, init, want, hit, what):
    """Per entry: an addressed entry grew by the fp64 sum to TABLE_TOL relative, every other entry keeps its initial bits."""
    got = tab.values()
    delta = got - init
    print(f"{what}: largest relative deviation of an entry {float(((delta - want).abs()[hit] / want.abs()[hit]).max()) if bool(hit.any()) else 0.0:.3e}")
    off = hit & ~((delta - want).abs() <= TABLE_TOL * want.abs())
    same = bits(got).reshape(got.shape) == bits(init).reshape(got.shape)
    bad = off | (~hit & ~same)
    if bool(bad.any()):
        s, b = (int(v) for v in bad.nonzero()[0])
        kind = f"grew by {delta[s, b].item()!r}, the fp64 sum is {want[s, b].item()!r}" if bool(hit[s, b]) else \
            f"is not addressed and changed from {init[s, b].item()!r} to {got[s, b].item()!r}"
        raise AssertionError(f"{what}: {int(bad.sum())} entries are wrong, the first at (slot, sample) = ({s}, {b}): it {kind}")


def check_same_bits(a, b, what):
    X.check_exact(a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1]), what, bitwise=True)


# ---- runners: forward family -----------------------------------------------------------------------------------------------------
def run_fwd_select(be, dev, shape, T, figures=None, what=""):
    """mmdyn_tconv_out3_bn_fwd on the six selection sets (gamma pattern s % 2)."""
    i = inputs(shape, T)
    for s in range(6):
        a, M = act_ref(F64, i, s % 2)
        ref, Mx, valid = select_logits(a, M, shape, s)
        w = f"{what}tconv_out3_bn_fwd {shape} {T} weight set {s}"
        L = Launch(be, dev, "fwd", i, s % 2, SETS[s][0], what=w)
        check_logits(L.logits(), ref, Mx, valid, C_ACT, w, figures)


def run_dense(be, dev, shape, T, figures=None, what=""):
    """The dense family: mmdyn_tconv_out3_bn_fwd and the logits the three loss forms publish (all groups), both gamma patterns."""
    i = inputs(shape, T)
    for p in (0, 1):
        ref, Mx = dense_logits(*act_ref(F64, i, p), shape, F64)
        for entry in ("fwd",) + ENTRIES:
            w = f"{what}{entry} {shape} {T} dense weights, gamma pattern {p}"
            L = Launch(be, dev, entry, i, p, DENSE_W, lgroup=-1, what=w)
            check_logits(L.logits(), ref, Mx, None, C_DENSE, f"{w}: logits", figures)


def loss_combos(entry, G):
    """(mask channels, logits_group or None, gradient buffer) of one entry point; the weight set cycles with the combination."""
    return [(mc, lg, dl) for mc in (0, 1, 3) for lg in [None, -1] + list(range(G)) for dl in ((True, False) if entry == "bce" else (True,))]


def run_loss(be, dev, shape, T, entry, figures=None, what=""):
    """One loss entry point on selection-family logits: dlogit per element, exact zeros, published logits bit-identical to
    mmdyn_tconv_out3_bn_fwd's, tables per entry, rows against the batch launch."""
    i = inputs(shape, T)
    G, Bg, Hi, Wi = shape
    slots = slots_of(G)
    fwd, last = {}, {}
    for k, (mc, lg, want_dl) in enumerate(loss_combos(entry, G)):
        s = k % 6
        p = s % 2
        w = f"{what}{entry} {shape} {T} weight set {s} mask_c={mc} logits_group={lg} dlogit={int(want_dl)}"
        a, M = act_ref(F64, i, p)
        x, Mx, valid = select_logits(a, M, shape, s)
        assert bool(torch.isfinite(x).all())
        lr = loss_ref(F64, x, i, mc, slots, i.w_rec if entry == "rows_grad" else torch.ones(Bg), logit_bound(x, Mx))
        L = Launch(be, dev, entry, i, p, SETS[s][0], lgroup=lg, mask_c=mc, slots=slots, want_dl=want_dl, what=w)
        if L.dl is not None:
            check_dlogit(L.dlogit(), lr, f"{w}: dlogit", figures)
        if lg is not None:
            if s not in fwd:
                fwd[s] = Launch(be, dev, "fwd", i, p, SETS[s][0], what=f"{w}: mmdyn_tconv_out3_bn_fwd").logits()
            check_same_bits(L.logits(), fwd[s] if lg < 0 else fwd[s][lg * Bg:(lg + 1) * Bg], f"{w}: logits against mmdyn_tconv_out3_bn_fwd's")
        want, hit = table_ref(lr["rows"], slots, entry != "bce")
        check_table(L.loss, L.init, want, hit, f"{w}: loss table")
        want_u, _ = table_ref(lr["rows_u"], slots, entry != "bce")
        check_table(L.unm, L.init, want_u, hit & bool(mc), f"{w}: unmasked table")
        last[mc] = (s, L)
    if entry != "bce":      # the rows of a slot add up to the slot of the batch launch (fp64 atomics: SAME_TOL)
        for mc, (s, L) in last.items():
            w = f"{what}{entry} {shape} {T} weight set {s} mask_c={mc}: rows summed over the samples against mmdyn_tconv_out3_bn_bce"
            Lb = Launch(be, dev, "bce", i, s % 2, SETS[s][0], mask_c=mc, slots=slots, want_dl=False, what=w)
            for tab_r, tab_b in ((L.loss, Lb.loss),) + (((L.unm, Lb.unm),) if mc else ()):
                r, b = L.delta(tab_r).sum(1, keepdim=True), Lb.delta(tab_b)
                assert bool(((r - b).abs() <= SAME_TOL * b.abs()).all()), f"{w}: {r.reshape(-1).tolist()} against {b.reshape(-1).tolist()}"


def run_identities(be, dev, shape, T, what=""):
    """mmdyn_tconv_out3_bn_bce_rows_grad with w_rec = 1 gives the dlogit bits of mmdyn_tconv_out3_bn_bce; with a mask of all ones
    the bits of the launch without a mask."""
    i = inputs(shape, T)
    G, Bg, Hi, Wi = shape
    for mc in (0, 1, 3):
        s = (mc + 2) % 6
        w = f"{what}{shape} {T} weight set {s} mask_c={mc}"
        a = Launch(be, dev, "bce", i, s % 2, SETS[s][0], mask_c=mc, what=w).dlogit()
        b = Launch(be, dev, "rows_grad", i, s % 2, SETS[s][0], mask_c=mc, w_rec=torch.ones(Bg), what=w).dlogit()
        check_same_bits(b, a, f"{w}: dlogit of rows_grad with w_rec = 1 against mmdyn_tconv_out3_bn_bce's")
    plain = Launch(be, dev, "rows_grad", i, 1, SETS[1][0], lgroup=-1, what=what)
    for mc in (1, 3):
        w = f"{what}{shape} {T} rows_grad with a mask of ones, {mc} channels"
        ones = Launch(be, dev, "rows_grad", i, 1, SETS[1][0], lgroup=-1, mask_c=mc, mask=torch.ones(Bg, mc, 2 * Hi, 2 * Wi), what=w)
        check_same_bits(ones.dlogit(), plain.dlogit(), f"{w}: dlogit against the launch without a mask")
        check_same_bits(ones.logits(), plain.logits(), f"{w}: logits against the launch without a mask")


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
def wgrad_inputs(shape, T):
    G, Bg, Hr = shape
    return inputs((G, Bg, Hr, Hr), T)


def units_of(shape):
    G, Bg, Hr = shape
    return G * Bg * Hr * (Hr // 32)


def chunk_values(be, shape):
    """{label: chunks}: 1, the recommended value, one that does not divide the unit count, one whose rows_per_chunk is no multiple
    of 4, one with a group boundary inside a chunk (G > 1), more blocks than units.  The properties are asserted."""
    G, Bg, Hr = shape
    U = units_of(shape)
    per = lambda c: -(-U // c)
    v = {"one": 1, "recommended": be.wgrad_chunks(IM2COL3, G * Bg * Hr * Hr, 32, 64), "no divisor": next(c for c in range(5, 64) if U % c)}
    v["ragged"] = next(c for c in range(6, 64) if per(c) % 4 and c not in v.values())
    if G > 1:
        bnd = Bg * Hr * (Hr // 32)
        v["group boundary"] = next(c for c in range(2, 64) if bnd % per(c) and c not in v.values())
        assert bnd % per(v["group boundary"]) and per(v["group boundary"]) > 1
    v["surplus"] = U + 3
    assert U % v["no divisor"] and per(v["ragged"]) % 4 and v["recommended"] >= 1
    return v


def probes(shape, chunks):
    """Up to 12 pixels (b, co, oy, ox) of the [Bt][3][2Hr][2Hr] gradient, one per (output channel, row parity, column parity)
    class: the four corners (first / last sample of a group), an edge, interior pixels, the columns on either side of a 64-pixel
    segment, the first pixel of the first unit and the last pixel of the last unit of the middle chunk."""
    G, Bg, Hr = shape
    Bt, S, segs, U = G * Bg, 2 * Hr, Hr // 32, units_of(shape)
    per = -(-U // chunks)
    c = min(chunks, -(-U // per)) // 2
    first, last = c * per, min(U, (c + 1) * per) - 1
    unit = lambda u: (u // (Hr * segs), (u % (Hr * segs)) // segs, u % segs)         # (sample, row, segment)
    (b0, y0, s0), (b1, y1, s1) = unit(first), unit(last)
    px = [(0, 0, 0, 0), (Bt - 1, 0, 0, S - 1), (Bg - 1, 0, S - 1, 0), (Bg % Bt, 0, S - 1, S - 1),
          (0, 1, 0, 10), (Bt - 1, 1, 8, 63), (0, 1, 9, 64 % S), (Bt // 2, 1, 13, 21),
          (b0, 2, 2 * y0, 64 * s0), (b1, 2, 2 * y1 + 1, 64 * s1 + 63), (0, 2, 20, 127 % S), (Bt - 1, 2, 21, 128 % S)]
    return px, (first, last)


def wgrad_select_ref(a, M, shape, px, vals):
    """(ref, M, units hit) [32][64] fp64: entry (ci, co 16 + kh 4 + kw) = value * a[b][iy][ix][ci] for the taps of the pixel's
    class, 0 where the tap leaves the image and everywhere else (columns 48..63 included)."""
    G, Bg, Hr = shape
    a4, M4 = a.reshape(G * Bg, Hr, Hr, 32), M.reshape(G * Bg, Hr, Hr, 32)
    ref, Mo, hit = torch.zeros(32, 64, dtype=a.dtype), torch.zeros(32, 64, dtype=a.dtype), set()
    for (b, co, oy, ox), v in zip(px, vals.tolist()):
        for kh in ((oy + 1) % 2, (oy + 1) % 2 + 2):
            for kw in ((ox + 1) % 2, (ox + 1) % 2 + 2):
                iy, ix = (oy + 1 - kh) // 2, (ox + 1 - kw) // 2
                if 0 <= iy < Hr and 0 <= ix < Hr:
                    col = co * 16 + kh * 4 + kw
                    assert not bool(Mo[:, col].any()), "broken case: two probe pixels hit one entry"
                    ref[:, col], Mo[:, col] = v * a4[b, iy, ix], abs(v) * M4[b, iy, ix]
                    hit.add((b * Hr + iy) * (Hr // 32) + ix // 32)
    return ref, Mo, hit


def _wgrad_launch(be, dev, i, p, Gt, shape, chunks, what):
    G, Bg, Hr = shape
    P = X.Guarded(chunks * 32, 64, F32, dev)
    be.wgrad_out3_bn(i.y.to(dev), i.mean.to(dev), i.rstd.to(dev), gamma_of(i, p).to(dev), i.beta.to(dev), Gt.to(dev),
                     P.view(chunks, 32, 64), G, Bg, Hr, chunks)
    _sync(dev)
    P.check(f"{what}: partial")
    slabs = P.values().reshape(chunks, 32, 64)
    U = units_of(shape)
    used = -(-U // -(-U // chunks))
    X.check_exact(slabs[used:].reshape(-1, 64), torch.zeros((chunks - used) * 32, 64), f"{what}: the slabs past the last unit")
    return slabs


def run_wgrad_select(be, dev, shape, T, label, figures=None, what=""):
    """mmdyn_wgrad_out3_bn on a one-hot Gt, one `chunks` value."""
    G, Bg, Hr = shape
    i = wgrad_inputs(shape, T)
    chunks = chunk_values(be, shape)[label]
    px, _ = probes(shape, chunks)
    for p in (0, 1):
        vals = X.pow2(12, 700 + p)
        Gt = torch.zeros(G * Bg, 3, 2 * Hr, 2 * Hr)
        for (b, co, oy, ox), v in zip(px, vals.tolist()):
            Gt[b, co, oy, ox] = v
        ref, M, _ = wgrad_select_ref(*act_ref(F64, i, p), shape, px, vals)
        w = f"{what}wgrad_out3_bn {shape} {T} chunks={chunks} ({label}) one-hot Gt, gamma pattern {p}"
        slabs = _wgrad_launch(be, dev, i, p, Gt, shape, chunks, w)
        got = slabs.double().sum(0)
        assert bool((got.float().double() == got).all()), f"{w}: two slabs hold the same entry"
        check_rule(got.float(), ref, M, F32, C_ACT, f"{w}: partial summed over the slabs", figures)
        X.check_exact(got.float()[M == 0].reshape(1, -1), torch.zeros(1, int((M == 0).sum())), f"{w}: the entries no probe pixel reaches")


_WDENSE = {}


def wgrad_dense_ref(shape, T, p, dt=F64):
    """(Gt, ref, M): Gt integer in [-3, 3]; ref [32][64] the autograd weight gradient of F.conv_transpose2d in dtype dt, M the same
    of (|gamma xhat| + |beta|) and |Gt| (fp64)."""
    key = (tuple(shape), T, p, dt)
    if key not in _WDENSE:
        G, Bg, Hr = shape
        i = wgrad_inputs(shape, T)
        Gt = X.ints((G * Bg, 3, 2 * Hr, 2 * Hr), 710 + p)

        def grad(a, gt, d):
            W = torch.zeros(32, 3, 4, 4, dtype=d, requires_grad=True)
            y = F.conv_transpose2d(a.to(d).reshape(G * Bg, Hr, Hr, 32).permute(0, 3, 1, 2), W, stride=2, padding=1)
            out = torch.zeros(32, 64, dtype=d)
            out[:, :48] = torch.autograd.grad(y, W, gt.to(d))[0].reshape(32, 48)
            return out
        a, M = act_ref(dt, i, p)
        _WDENSE[key] = (Gt, grad(a, Gt, dt), grad(act_ref(F64, i, p)[1], Gt.abs(), F64))
    return _WDENSE[key]


def run_wgrad_dense(be, dev, shape, T, label, figures=None, what=""):
    """mmdyn_wgrad_out3_bn on an integer Gt, one `chunks` value, both gamma patterns."""
    i = wgrad_inputs(shape, T)
    chunks = chunk_values(be, shape)[label]
    for p in (0, 1):
        Gt, ref, M = wgrad_dense_ref(shape, T, p)
        w = f"{what}wgrad_out3_bn {shape} {T} chunks={chunks} ({label}) dense Gt, gamma pattern {p}"
        slabs = _wgrad_launch(be, dev, i, p, Gt, shape, chunks, w)
        check_rule(slabs.double().sum(0).float(), ref, M, F32, C_W, f"{w}: partial summed over the slabs", figures)


def run_wgrad_refused(be, dev, T, what=""):
    """Every size but square 32 / 64 / 128 is MMDYN_ERR_SHAPE (the entry point has one extent: a non-square image cannot be
    stated); nothing is launched, the JUNK of the destination stays."""
    for Hr in WGRAD_REFUSED:
        y = torch.zeros(Hr * Hr, 32).to(T).to(dev)
        z = torch.zeros(32, device=dev)
        P = X.Guarded(4 * 32, 64, F32, dev)
        try:
            be.wgrad_out3_bn(y, z.reshape(1, 32), z.reshape(1, 32) + 1, z + 1, z, torch.zeros(1, 3, 2 * Hr, 2 * Hr, device=dev), P.view(4, 32, 64),
                             1, 1, Hr, 4)
        except MmdynError as e:
            assert "MMDYN_ERR_SHAPE" in str(e), f"{what}Hr={Hr}: {e}"
        else:
            raise AssertionError(f"{what}mmdyn_wgrad_out3_bn accepted Hr = {Hr}")
        _sync(dev)
        X.check_exact(P.values(), torch.full((4 * 32, 64), P.values()[0, 0].item()), f"{what}Hr={Hr}: partial of a refused launch")
        P.check(f"{what}Hr={Hr}: partial")


# ---- the fp32 twin: how the constants were measured -------------------------------------------------------------------------------
def _ratio(r32, ref, M, normal_only=False):
    """Largest |r32 - ref| / (2^-24 M) over the elements with M > 0; normal_only (the dlogit measurement alone): of those, the
    elements whose reference is a normal fp32 number."""
    ok = (M > 0) & (ref.abs() >= 2.0 ** -126) if normal_only else M > 0
    return float(((r32.double() - ref).abs()[ok] / (TWO_M24 * M[ok])).max())


def twin_figures(T):
    """[(name, c, largest |r32 - ref| / (2^-24 M))] of the plain torch-fp32 evaluation over every input above, storage type T."""
    rows = []
    for shape in LOSS_SHAPES + [(G, Bg, Hr, Hr) for G, Bg, Hr in WGRAD_SHAPES]:
        i = inputs(shape, T)
        for p in (0, 1):
            a, M = act_ref(F64, i, p)
            a32 = act_ref(F32, i, p)[0]
            rows.append((f"activation {shape} pattern {p}", C_ACT, _ratio(a32, a, M)))
            if shape[2] > 48:
                continue
            ref, Mx = dense_logits(a, M, shape, F64)
            rows.append((f"dense logits {shape} pattern {p}", C_DENSE, _ratio(dense_logits(a32, M, shape, F32)[0], ref, Mx)))
        if shape[2] > 48:
            continue
        worst = 0.0
        for s in range(6):
            x32 = select_logits(*act_ref(F64, i, s % 2), shape, s)[0].float()
            for mc in (0, 1, 3):
                lr = loss_ref(F64, x32.double(), i, mc, slots_of(shape[0]), i.w_rec)
                worst = max(worst, _ratio(loss_ref(F32, x32, i, mc, slots_of(shape[0]), i.w_rec)["d"], lr["d"], lr["Md"], normal_only=True))
        rows.append((f"dlogit {shape}", C_D, worst))
    for shape in WGRAD_SHAPES:
        for p in (0, 1):
            _, ref, M = wgrad_dense_ref(shape, T, p)
            rows.append((f"dense weight gradient {shape} pattern {p}", C_W, _ratio(wgrad_dense_ref(shape, T, p, F32)[1], ref, M)))
    return rows


def measure():
    worst = {}
    for T in (F32, BF16, F16):
        for name, c, ratio in twin_figures(T):
            print(f"{str(T):16s} {name:60s} c = {c:5.1f}  measured {ratio:6.2f}")
            if ratio > worst.get(c, ("", 0.0))[1]:
                worst[c] = (f"{name}, {T}", ratio)
    for c, (name, ratio) in worst.items():
        print(f"c = {c:5.1f}: largest {ratio:.2f} ({name})")


if __name__ == "__main__":
    measure()
