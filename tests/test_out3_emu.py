"""The per-element checks of tests/out3_cases.py on the CPU: (i) every case that tests/test_out3_gpu.py holds the kernels to, on the
contract emulation; (ii) the plain torch-fp32 evaluation of every formula stays within a quarter of its bound and every constant is
4 x its measured maximum; (iii) the preconditions of the cases, on the reference alone; (iv) the checks bite: a plain fp32
evaluation of the five entry points passes every runner, and each of its deliberately wrong variants is reported."""
import pytest
import torch
import torch.nn.functional as F

import out3_cases as O
from emu_backend import EmuBackend
from emu_backend_weighted import EmuBackendWeighted
from mmdyn_hip._lib import MmdynError
from out3_cases import F32, F64

EMU = EmuBackendWeighted()
DEV = "cpu"
TYPE_IDS = list(O.TYPES)


@pytest.fixture(params=TYPE_IDS)
def T(request):
    EMU.precision = request.param
    yield O.TYPES[request.param]
    EMU.precision = "fp32"


# ---- (i) the emulation passes every runner ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", O.FWD_SHAPES)
def test_forward_selection_and_dense(shape, T):
    O.run_fwd_select(EMU, DEV, shape, T)
    O.run_dense(EMU, DEV, shape, T)


@pytest.mark.parametrize("entry", O.ENTRIES)
@pytest.mark.parametrize("shape", O.LOSS_SHAPES)
def test_loss_epilogue(shape, entry, T):
    O.run_loss(EMU, DEV, shape, T, entry)


@pytest.mark.parametrize("shape", [O.FWD_SHAPES[1], O.FWD_SHAPES[2], O.SLOTS_SHAPE])
def test_identities_of_the_weighted_form(shape, T):
    O.run_identities(EMU, DEV, shape, T)


@pytest.mark.parametrize("shape", O.WGRAD_SHAPES)
def test_weight_gradient(shape, T):
    for label in O.chunk_values(EMU, shape):
        O.run_wgrad_select(EMU, DEV, shape, T, label)
        O.run_wgrad_dense(EMU, DEV, shape, T, label)


def test_weight_gradient_refuses_other_sizes():
    O.run_wgrad_refused(EMU, DEV, F32)


# ---- (ii) the fp32 twin ----------------------------------------------------------------------------------------------------------
_FIG = {}


def _figures(name):
    if name not in _FIG:
        _FIG[name] = O.twin_figures(O.TYPES[name])
    return _FIG[name]


@pytest.mark.parametrize("name", TYPE_IDS)
def test_fp32_evaluation_is_within_a_quarter_of_the_bound(name):
    rows = _figures(name)
    assert len(rows) >= 40
    for what, c, ratio in rows:
        print(f"{name} {what}: c = {c}, fp32 evaluation at {ratio:.2f} x 2^-24 M")
        assert ratio <= c / 4, f"{what} ({name}): the fp32 evaluation reaches {ratio:.2f} x 2^-24 M, more than a quarter of c = {c}"


def test_every_constant_is_four_times_its_measured_maximum():
    worst = {}
    for name in TYPE_IDS:
        for _, c, ratio in _figures(name):
            worst[c] = max(worst.get(c, 0.0), ratio)
    assert sorted(worst) == sorted([O.C_ACT, O.C_DENSE, O.C_D, O.C_W])
    for c, ratio in worst.items():
        assert 4 * ratio <= c < 4 * ratio + 1, (c, ratio)


# ---- (iii) preconditions, on the reference alone -----------------------------------------------------------------------------------
ALL_SHAPES = O.LOSS_SHAPES + [(G, Bg, Hr, Hr) for G, Bg, Hr in O.WGRAD_SHAPES]


def _reach(shape, T):
    """The preconditions of one (shape, type) -> the extremes of u on the wide channels and of the selection logits."""
    i = O.inputs(shape, T)
    us, xs = [], []
    G, Bg, Hi, Wi = shape
    assert i.y.dtype == T and (G == 1 or not torch.equal(i.mean[0], i.mean[1])) and (G == 1 or not torch.equal(i.rstd[0], i.rstd[1]))
    assert bool((i.beta > 0).any()) and bool((i.beta < 0).any())
    assert bool((i.target == 0).any()) and bool((i.target == 1).any()) and float(i.target.min()) >= 0 and float(i.target.max()) <= 1
    assert all(set(m.unique().tolist()) == {0.0, 1.0} for m in i.masks.values()) and i.w_rec.unique().numel() == Bg
    big = torch.arange(32) % 5 == 0
    for p in (0, 1):
        gm = O.gamma_of(i, p)
        assert bool((gm[0::2] > 0).all() if p == 0 else (gm[0::2] < 0).all()) and bool((gm[1::2] * gm[0::2] < 0).all())
        xh = (i.y.double().reshape(G, -1, 32) - i.mean.double()[:, None]) * i.rstd.double()[:, None]
        u = gm.double() * xh + i.beta.double()
        assert float(u[..., big].max()) >= 24 and float(u[..., big].min()) <= -24, (float(u[..., big].min()), float(u[..., big].max()))
        us += [float(u[..., big].min()), float(u[..., big].max())]
        assert float(u[..., big].abs().max()) <= 34 and float(u[..., ~big].abs().max()) <= 3
        a, M = O.act_ref(F64, i, p)
        assert bool(torch.isfinite(a).all()) and bool((M > 0).all())
    if Hi <= 48:
        lo, hi = 0.0, 0.0
        for s in range(6):
            x, Mx, valid = O.select_logits(*O.act_ref(F64, i, s % 2), shape, s)
            assert bool(torch.isfinite(x).all()) and bool((~valid).any()) and bool((x[~valid] == 0).all()) and bool((Mx >= x.abs()).all())
            lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
        # exp(-|x|) underflows (|x| > 104); at both ends sigmoid - t is -t or 1 - t to the last bit (sigmoid(-75) = 3e-33)
        assert hi >= 175 and lo <= -75 and max(hi, -lo) <= 280, (lo, hi)
        xs += [lo, hi]
        assert O.slots_of(G).count(-1) == (G > 1) and (G != 4 or O.slots_of(G) == [5, -1, 0, 0])
    return us, xs


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_inputs_reach_the_stated_ranges(shape, T):
    _reach(shape, T)


def test_over_the_shapes_the_inputs_reach_the_documented_extremes():
    """u beyond +-30 and logits from -120 to +240, as tests/out3_cases.py and docs/LAB_NOTES.md state (fp32 y; the 16-bit types give
    the same figures to the first decimal)."""
    us, xs = [], []
    for shape in ALL_SHAPES:
        u, x = _reach(shape, F32)
        us, xs = us + u, xs + x
    assert min(us) <= -30 and max(us) >= 30, us
    assert min(xs) <= -120 and max(xs) >= 240, xs


def test_the_six_weight_sets_cover_the_sixteen_taps():
    taps = set()
    for w, tap, ci, scale in O.SETS:
        assert int((w != 0).sum()) == 3 and bool((scale.abs().log2().abs() <= 3).all())
        assert all(float(w[ci[k], k, tap[k] >> 2, tap[k] & 3]) == float(scale[k]) for k in range(3))
        taps |= set(tap.tolist())
    assert taps == set(range(16))
    assert {int(c) % 5 == 0 for _, _, ci, _ in O.SETS for c in ci} == {True, False}      # channels of both ranges of u are selected


@pytest.mark.parametrize("shape", O.WGRAD_SHAPES)
def test_probe_pixels_hit_disjoint_entries_and_the_stated_places(shape):
    G, Bg, Hr = shape
    S, segs, U = 2 * Hr, Hr // 32, O.units_of(shape)
    values = O.chunk_values(EMU, shape)
    assert len(set(values.values())) == len(values) == (6 if G > 1 else 5) and values["surplus"] > U
    i = O.wgrad_inputs(shape, F32)
    for label, chunks in values.items():
        px, (first, last) = O.probes(shape, chunks)
        assert len({(co, oy % 2, ox % 2) for _, co, oy, ox in px}) == 12
        assert all(0 <= b < G * Bg and 0 <= oy < S and 0 <= ox < S for b, _, oy, ox in px)
        ref, M, hit = O.wgrad_select_ref(*O.act_ref(F64, i, 0), shape, px, O.X.pow2(12, 700))
        assert first in hit and last in hit and first % -(-U // chunks) == 0
        assert int((M > 0).any(0).sum()) <= 48 and not bool(M[:, 48:].any())
        where = {(oy, ox) for _, _, oy, ox in px}
        assert {(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)} <= where
        cols = {ox for _, ox in where}
        assert segs == 1 or {63, 64} <= cols
        assert segs < 4 or {127, 128} <= cols
        samples = {b for b, _, _, _ in px}
        assert {0, Bg - 1, G * Bg - 1, Bg % (G * Bg)} <= samples


# ---- (iv) the checks bite --------------------------------------------------------------------------------------------------------
class Plain:
    """The five entry points as a plain torch-fp32 evaluation of the documented formulas; `defect` names ONE deliberate mistake."""
    precision = "fp32"

    def __init__(self, defect=None):
        self.defect = defect

    def wgrad_chunks(self, *a):
        return EMU.wgrad_chunks(*a)

    @staticmethod
    def _swish(u):
        return u / (1 + torch.exp(-u))

    def _full(self, y, mean, rstd, gamma, beta, w, G, Bg, Hi, Wi):
        Bt = G * Bg
        if self.defect == "group 0's statistics for every sample":
            mean, rstd = mean[:1].expand(G, 32), rstd[:1].expand(G, 32)
        y4 = y.float().reshape(G, Bg, Hi, Wi, 32)
        pad = self.defect == "padding applied before the activation"
        if pad:
            y4 = F.pad(y4, (0, 0, 1, 1, 1, 1))
        a = self._swish(gamma * ((y4 - mean.reshape(G, 1, 1, 1, 32)) * rstd.reshape(G, 1, 1, 1, 32)) + beta)
        a = a.reshape(Bt, Hi + 2 * pad, Wi + 2 * pad, 32).permute(0, 3, 1, 2)
        full = F.conv_transpose2d(a, w.reshape(32, 3, 4, 4), stride=2, padding=1)
        if pad:
            full = full[:, :, 2:-2, 2:-2]
        if self.defect == "a halo column dropped at a tile boundary":
            for t in range(1, Wi // 16):
                left = torch.zeros_like(a)
                left[..., 16 * t - 1] = a[..., 16 * t - 1]
                full[..., 32 * t:] -= F.conv_transpose2d(left, w.reshape(32, 3, 4, 4), stride=2, padding=1)[..., 32 * t:]
        return full.contiguous()

    def tconv_out3_bn_fwd(self, y, mean, rstd, gamma, beta, w, out, G, Bg, Hi, Wi):
        out.reshape(-1).copy_(self._full(y, mean, rstd, gamma, beta, w, G, Bg, Hi, Wi).reshape(-1))

    def _loss(self, full, logits, lgroup, target, dlogit, w_rec, loss, unm, slots, gs, G, Bg, mask, mask_c, per_sample):
        x = full.reshape(G, Bg, *full.shape[1:])
        smp = torch.arange(Bg).expand(G, Bg)
        other = (smp + torch.arange(G)[:, None]) % Bg             # (the sample a [Bg] table gives when it is indexed by the row b)
        t = target[other if self.defect == "the target indexed by b instead of smp" else smp]
        mk = torch.ones(())
        if mask is not None:
            m = mask[:, :1] if self.defect == "mask channel 0 used when mask_c = 3" else mask
            mk = m.expand(Bg, 3, *m.shape[2:])[other if self.defect == "the mask indexed by b instead of smp" else smp]
        w = torch.ones(Bg) if w_rec is None else w_rec
        w = w[other if self.defect == "w_rec indexed by b instead of smp" else smp].reshape(G, Bg, 1, 1, 1)
        xm, tm = x * mk, t * mk
        sig = 1 / (1 + torch.exp(-xm))
        d = (mk * (sig - tm) * torch.tensor(gs)) * w
        elem = F.binary_cross_entropy_with_logits(xm, tm, reduction="none").double().sum((2, 3, 4))
        elem_u = F.binary_cross_entropy_with_logits(x, t, reduction="none").double().sum((2, 3, 4))
        dl = None if dlogit is None else dlogit.reshape(G, Bg, *full.shape[1:])
        shift = self.defect == "the rows sum added to the neighbouring sample"
        for g, slot in enumerate(slots):
            if slot < 0:
                if dl is not None and self.defect != "a discarded group's dlogit left unwritten":
                    dl[g].zero_()
                continue
            if dl is not None:
                dl[g] = d[g]
            for tab, e in ((loss, elem), (unm if mask is not None else None, elem_u)):
                if tab is None:
                    continue
                if per_sample:
                    tab[slot] += e[g].roll(1) if shift else e[g]
                else:
                    tab[slot] += e[g].sum()
        if logits is not None:
            src = full if lgroup < 0 else full[lgroup * Bg:(lgroup + 1) * Bg]
            logits.reshape(-1).copy_(src.reshape(-1))
            if lgroup >= 0 and self.defect == "one logit written one row past a [Bg] out":
                torch.as_strided(logits, (1,), (1,), logits.storage_offset() + logits.numel() + 5).fill_(float(src.reshape(-1)[5]))

    def tconv_out3_bn_bce(self, y, mean, rstd, gamma, beta, w, logits, lgroup, target, dlogit, loss_slots, slots, gs, G, Bg, Hi, Wi,
                          mask=None, mask_channels=1, unmasked_slots=None):
        full = self._full(y, mean, rstd, gamma, beta, w, G, Bg, Hi, Wi)
        self._loss(full, logits, lgroup, target, dlogit, None, loss_slots, unmasked_slots, slots, gs, G, Bg, mask, mask_channels, False)

    def tconv_out3_bn_bce_rows(self, y, mean, rstd, gamma, beta, w, logits, lgroup, target, loss_rows, slots, G, Bg, Hi, Wi, mask=None,
                               mask_channels=1, unmasked_rows=None):
        full = self._full(y, mean, rstd, gamma, beta, w, G, Bg, Hi, Wi)
        self._loss(full, logits, lgroup, target, None, None, loss_rows, unmasked_rows, slots, 0.0, G, Bg, mask, mask_channels, True)

    def tconv_out3_bn_bce_rows_grad(self, y, mean, rstd, gamma, beta, w, logits, lgroup, target, dlogit, w_rec, loss_rows, slots, gs, G,
                                    Bg, Hi, Wi, mask=None, mask_channels=1, unmasked_rows=None):
        full = self._full(y, mean, rstd, gamma, beta, w, G, Bg, Hi, Wi)
        self._loss(full, logits, lgroup, target, dlogit, w_rec, loss_rows, unmasked_rows, slots, gs, G, Bg, mask, mask_channels, True)

    def wgrad_out3_bn(self, y, mean, rstd, gamma, beta, Gt, partial, G, Bg, Hr, chunks):
        if Hr not in (32, 64, 128):
            raise MmdynError("mmdyn_wgrad_out3_bn failed: MMDYN_ERR_SHAPE (unsupported dimensions)")
        g = EmuBackend._unfold3(Gt, G * Bg, 2 * Hr, 2 * Hr)
        units = G * Bg * Hr * (Hr // 32)
        per = -(-units // chunks)
        grp = (torch.arange(units * 32) // (Hr * Hr)) // Bg
        p = partial.reshape(chunks, 32, 64)
        for c in range(chunks):
            lo, hi = min(units, c * per), min(units, (c + 1) * per)
            if self.defect == "a weight gradient that skips the last unit of a chunk" and hi > lo:
                hi -= 1
            rows = slice(lo * 32, hi * 32)
            gr = grp[rows]
            if self.defect == "a weight gradient that keeps the previous group's statistics across the boundary" and hi > lo:
                gr = gr[:1].expand(gr.numel())
            a = self._swish(gamma * ((y.float().reshape(-1, 32)[rows] - mean[gr]) * rstd[gr]) + beta)
            p[c] = a.t() @ g[rows]


BITE_SHAPE = (2, 2, 16, 32)
# defect -> (the runner that must report it, what its report says)
DEFECTS = {
    "padding applied before the activation": (lambda be: O.run_fwd_select(be, DEV, (1, 1, 16, 16), F32), r"tconv_out3_bn_fwd .*break rule 1"),
    "group 0's statistics for every sample": (lambda be: O.run_fwd_select(be, DEV, BITE_SHAPE, F32), r"tconv_out3_bn_fwd .*break rule 1"),
    "a halo column dropped at a tile boundary": (lambda be: O.run_fwd_select(be, DEV, BITE_SHAPE, F32), r"tconv_out3_bn_fwd .*break rule 1"),
    "the target indexed by b instead of smp": (lambda be: O.run_loss(be, DEV, O.SLOTS_SHAPE, F32, "rows_grad"), r"dlogit: \d+ of \d+ elements break rule 1"),
    "the mask indexed by b instead of smp": (lambda be: O.run_loss(be, DEV, O.SLOTS_SHAPE, F32, "rows_grad"), r"mask_c=1 .*dlogit"),
    "w_rec indexed by b instead of smp": (lambda be: O.run_loss(be, DEV, O.SLOTS_SHAPE, F32, "rows_grad"), r"dlogit: \d+ of \d+ elements break rule 1"),
    "mask channel 0 used when mask_c = 3": (lambda be: O.run_loss(be, DEV, BITE_SHAPE, F32, "bce"), r"mask_c=3 .*dlogit"),
    "a discarded group's dlogit left unwritten": (lambda be: O.run_loss(be, DEV, BITE_SHAPE, F32, "bce"), r"dlogit: \d+ of \d+ elements break rule 1"),
    "one logit written one row past a [Bg] out": (lambda be: O.run_loss(be, DEV, BITE_SHAPE, F32, "bce"), r"logits_group=0 .*logits: wrote outside its declared extent"),
    "the rows sum added to the neighbouring sample": (lambda be: O.run_loss(be, DEV, BITE_SHAPE, F32, "rows"), r"loss table: \d+ entries are wrong"),
    "a weight gradient that skips the last unit of a chunk": (lambda be: O.run_wgrad_select(be, DEV, (2, 2, 32), F32, "ragged"), r"one-hot Gt.*break rule 1"),
    "a weight gradient that keeps the previous group's statistics across the boundary":
        (lambda be: O.run_wgrad_select(be, DEV, (2, 2, 32), F32, "group boundary"), r"one-hot Gt.*break rule 1"),
}


def test_the_plain_fp32_evaluation_passes_every_runner():
    be = Plain()
    for shape in ((1, 1, 16, 16), BITE_SHAPE):
        O.run_fwd_select(be, DEV, shape, F32)
        O.run_dense(be, DEV, shape, F32)
    for entry in O.ENTRIES:
        O.run_loss(be, DEV, BITE_SHAPE, F32, entry)
        O.run_loss(be, DEV, O.SLOTS_SHAPE, F32, entry)
    O.run_identities(be, DEV, BITE_SHAPE, F32)
    for label in O.chunk_values(be, (2, 2, 32)):
        O.run_wgrad_select(be, DEV, (2, 2, 32), F32, label)
        O.run_wgrad_dense(be, DEV, (2, 2, 32), F32, label)
    O.run_wgrad_refused(be, DEV, F32)


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_a_wrong_emulation_is_reported(defect):
    run, says = DEFECTS[defect]
    with pytest.raises(AssertionError, match=says):
        run(Plain(defect))


@pytest.mark.parametrize("defect", ["a weight gradient that skips the last unit of a chunk",
                                    "a weight gradient that keeps the previous group's statistics across the boundary"])
def test_a_wrong_weight_gradient_is_reported_by_the_dense_check_too(defect):
    label = "ragged" if "skips" in defect else "one"
    with pytest.raises(AssertionError, match=r"dense Gt.*break rule 1"):
        O.run_wgrad_dense(Plain(defect), DEV, (2, 2, 32), F32, label)
