"""Ensemble quantiles on a real MI355X: mmdyn_ensemble_quantiles against the restatement of tests/quantile_cases.py (a sort and
single fp64 operations) on the existing kernel's bits of the prediction (mmdyn_rollout_feed with nothing observed), bit for bit;
ties, +-Inf and NaN samples; dirty destinations; bad arguments -- then ``MVAEInference.rollout(samples=N, quantiles=...)``: the
checks of tests/test_quantiles_emu.py on the HIP library, captured against eager on one Philox stream, and on dirty allocator
memory.  The reference has no rollout: nothing here comes from a golden file."""
import ctypes

import pytest
import torch

import dirty
import quantile_cases as QC
import rollout_cases as RC
import test_ensemble_emu as EE
import test_mixed_modal_emu as TMM
import test_quantiles_emu as QE
import test_rollout_emu as E
from mmdyn_hip import _lib, engine, layers, ops
from mmdyn_hip.engine import MVAEInference
from test_elbo_rows_gpu import RTOL_SUM          # (that file's constant, not a new one)
from test_rollout_gpu import gen

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
T, B, L, N = EE.T, EE.B, EE.L, EE.N
NMAX = QC.QUANTILE_N_MAX
Q1 = (0.4,)                                                      # one interpolated quantile
Q8 = (0.0, 1.0, 0.5, 0.5, 0.3, 0.77, 0.05, 0.95)                 # both ends, a repeated q, interpolated ones; not ascending


def shifted(shape, shift, fill=float("nan")):
    """fp32 ``shape`` on the device that starts ``shift`` floats past a 16-byte boundary."""
    n = 1
    for s in shape:
        n *= s
    t = torch.full((n + 4,), fill, device=DEV)[shift:shift + n].view(shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * shift
    return t


def operands(row_lens, n_s, Bk, Q, seed, shift=0):
    """Per group {src [N * B, n], out [Q, B, n], logits} on the device; ``shift``: every out starts that many floats past a 16-byte
    boundary.  The pose-sized group (7), the rows-sized group (1) and the second 12-float group hold plain signed values, the
    others logits (as tests/test_ensemble_gpu.py::operands)."""
    return [dict(src=(3.0 * gen(seed + g, n_s * Bk, n)).to(DEV), out=shifted((Q, Bk, n), shift),
                 logits=n not in (7, 1) and (g, n) != (1, 12)) for g, n in enumerate(row_lens)]


def prediction(groups, n_s, Bk):
    """p [N, B, n] per group: mmdyn_rollout_feed on the N * B rows with nothing observed -- the existing kernel's sigmoid bits."""
    ref = [dict(recon=g["src"], obs=None, out=torch.full_like(g["src"], float("nan")), logits=g["logits"], column=min(i, 2))
           for i, g in enumerate(groups)]
    HIP.rollout_feed(ref, None, n_s * Bk)
    return [r["out"].view((n_s, Bk) + tuple(r["out"].shape[1:])) for r in ref]


def run(groups, qs, n_s, Bk):
    lo, frac = QC.index_of(qs, n_s)
    for g in groups:
        g["out"].fill_(float("nan"))
    HIP.ensemble_quantiles(groups, lo, frac, n_s, Bk)
    return lo, frac


# the issue's operands: N = 1 on the element path; the quad path with the pose on the element path (B * 7 = 35); pose quads that
# straddle rows (B * 7 = 28); odd N past any unroll of 8, more items than a block, the rows-shaped group; destinations off the
# 16-byte boundary; N at and just below the constant; the real frame.  The kernel has ONE method for every N.
CASES = [((7,), 1, 1, 0), ((48, 48, 7), 3, 5, 0), ((48, 48, 7), 2, 4, 0), ((48, 48, 7, 1), 9, 37, 0), ((12, 12), 3, 3, 1),
         ((48,), NMAX, 2, 0), ((48,), NMAX - 1, 2, 0), ((12288, 12288, 7), 4, 2, 0)]


@pytest.mark.parametrize("qs", [Q1, Q8], ids=["Q1", "Q8"])
@pytest.mark.parametrize("row_lens,n_s,Bk,shift", CASES)
def test_kernel_has_the_bits_of_the_restatement(row_lens, n_s, Bk, shift, qs):
    """1. Every output element against sort + single fp64 operations on the prediction's bits."""
    groups = operands(row_lens, n_s, Bk, len(qs), 1040 + Bk + n_s, shift)
    lo, frac = run(groups, qs, n_s, Bk)
    for i, (g, p) in enumerate(zip(groups, prediction(groups, n_s, Bk))):
        want = QC.restate(p, lo, frac)
        assert not bool(torch.isnan(g["out"]).any()), i
        d = dirty.first_diff(g["out"], want)
        assert d is None, (i, d, g["out"].reshape(-1)[d].item(), want.reshape(-1)[d].item())
        if n_s > 1 and len(qs) > 1:
            assert not torch.equal(g["out"][0], g["out"][1]), i


def test_selected_values_have_the_sigmoid_bits_of_the_feed():
    """q = k / (N - 1), k = 0 .. N-1 (frac == 0 everywhere): the outputs are the N samples of the element, sorted -- for a logits
    group the bits mmdyn_rollout_feed writes for the same src."""
    n_s, Bk = 5, 6
    qs = tuple(k / (n_s - 1) for k in range(n_s))
    groups = operands((48, 7), n_s, Bk, n_s, 1060)
    lo, frac = run(groups, qs, n_s, Bk)
    assert lo == list(range(n_s)) and frac == [0.0] * n_s
    for g, p in zip(groups, prediction(groups, n_s, Bk)):
        assert dirty.first_diff(g["out"], torch.sort(p, dim=0).values) is None
    assert float(groups[0]["out"].min()) > 0.0 and float(groups[0]["out"].max()) < 1.0


def test_equal_values_infinities_and_zeros():
    """Samples that compare equal inside an element (a grid of few values, signed zeros among them) and +-Inf samples: the
    restatement's value everywhere (``==`` on the numbers: the sign of a zero result is the one thing left open), no NaN where no
    interpolation meets Inf - Inf, and with frac == 0 the infinities come out as ordinary values."""
    n_s, Bk, n = 9, 5, 12
    src = (torch.round(2.0 * gen(1070, n_s * Bk, n)) / 2.0).to(DEV)           # multiples of 0.5: many ties
    zeros = (src == 0).nonzero()[::2]
    src[zeros[:, 0], zeros[:, 1]] = -0.0
    src[1::7, 3], src[2::5, 4] = float("inf"), float("-inf")
    src.view(n_s, Bk, n)[:, 2, 7] = float("inf")                              # an element of N equal infinities
    for logits in (False, True):
        for qs in (Q8, tuple(k / 8 for k in range(8))):
            g = dict(src=src, out=shifted((8, Bk, n), 0), logits=logits)
            lo, frac = run([g], qs, n_s, Bk)
            want = QC.restate(prediction([g], n_s, Bk)[0], lo, frac)
            nan = torch.isnan(g["out"])
            assert torch.equal(nan, torch.isnan(want))                        # (Inf - Inf: a NaN, of either sign)
            d = QC.first_diff(g["out"].masked_fill(nan, 0.0), want.masked_fill(nan, 0.0))
            assert d is None, (logits, qs, d)
            if all(f == 0.0 for f in frac):
                assert not bool(nan.any())
    assert bool((src == 0).any()) and bool(torch.isinf(src).any())


def test_a_nan_sample_stays_in_its_element():
    """A NaN in one sample of one element makes all Q outputs of that element NaN; every other output keeps its bits."""
    row_lens, n_s, Bk = (48, 48, 7), 3, 5
    groups = operands(row_lens, n_s, Bk, 8, 1080)
    run(groups, Q8, n_s, Bk)
    first = [g["out"].clone() for g in groups]
    for gi, (n, b, i) in enumerate(((1, 1, 5), (0, 4, 47), (2, 3, 6))):
        groups[gi]["src"][n * Bk + b, i] = float("nan")
    run(groups, Q8, n_s, Bk)
    for gi, (b, i) in enumerate(((1, 5), (4, 47), (3, 6))):
        hit = torch.zeros_like(groups[gi]["out"], dtype=torch.bool)
        hit[:, b, i] = True
        out = groups[gi]["out"]
        assert bool(torch.isnan(out[hit]).all()) and not bool(torch.isnan(out[~hit]).any()), gi
        assert dirty.first_diff(out[~hit], first[gi][~hit]) is None, gi


def test_quantiles_on_dirty_destinations():
    """Zero-, NaN- and junk-filled out (tests/dirty.py): the same bits, no ``approx``; the inputs are not written."""
    row_lens, n_s, Bk = (48, 48, 7, 1), 9, 5
    src = operands(row_lens, n_s, Bk, 8, 1090)
    lo, frac = QC.index_of(Q8, n_s)

    def quantiles(backend, srcs, outs):
        backend.ensemble_quantiles([dict(src=s, out=o, logits=g["logits"]) for s, o, g in zip(srcs, outs, src)], lo, frac, n_s, Bk)
    args = ([g["src"] for g in src], [torch.empty(8, Bk, n) for n in row_lens])
    runs = dirty.run_dirty(HIP, quantiles, args, outs=[1], device=DEV)
    dirty.assert_same_bits(runs, what="ensemble_quantiles: ")


def test_quantiles_reject_bad_arguments():
    """MMDYN_ERR_NULL / _SHAPE / _RANGE from the raw entry point, before any launch."""
    lib, t = HIP.lib, torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    # per group (stride 1024 bytes), N = B = Q = 2 and rows of 4 floats: src [2][8] at +0 (64 bytes), out [2][8] at +128

    def call(G=1, Q=2, n_s=2, Bk=2, **over):
        a = _lib.QuantileGroups()
        for g in range(4):
            a.src[g], a.out[g], a.row_len[g], a.logits[g] = p + 1024 * g, p + 1024 * g + 128, 4, g & 1
        for j in range(8):
            a.lo[j], a.frac[j] = (min(j & 1, max(n_s - 1, 0)), 0.25 * (j & 3)) if j < Q else (-7, float("nan"))    # past Q: not looked at
        for k, (g, v) in over.items():
            getattr(a, k)[g] = v
        return lib.mmdyn_ensemble_quantiles(ctypes.addressof(a), G, Q, n_s, Bk, None)
    assert lib.mmdyn_ensemble_quantiles(None, 1, 1, 1, 1, None) == -2
    assert call(src=(0, None)) == -2 and call(out=(0, None)) == -2 and call(G=2, out=(1, None)) == -2 and call(G=3, src=(2, None)) == -2
    assert call(G=0) == -1 and call(G=5) == -1 and call(Q=0) == -1 and call(Q=9) == -1 and call(n_s=0) == -1 and call(Bk=0) == -1
    assert call(row_len=(0, 0)) == -1 and call(G=2, row_len=(1, -4)) == -1
    assert call(lo=(0, -1)) == -1 and call(lo=(1, 2)) == -1 and call(n_s=1, Bk=4, lo=(1, 1)) == -1
    assert call(frac=(0, 1.0)) == -1 and call(frac=(1, -0.125)) == -1 and call(frac=(1, float("nan"))) == -1
    assert call(frac=(0, float("inf"))) == -1
    assert call(out=(0, p)) == -1 and call(out=(0, p + 60)) == -1 and call(out=(0, p - 60)) == -1       # out on its own src
    assert call(G=2, out=(0, p + 1024 + 32)) == -1 and call(G=2, out=(1, p + 32)) == -1                 # ... on another group's
    assert call(G=2, out=(1, p + 128 + 32)) == -1 and call(G=3, out=(2, p + 1024 + 128 - 32)) == -1     # ... on another out
    assert call(n_s=NMAX + 1, Bk=1) == -3
    assert call(n_s=NMAX, Bk=1, row_len=(0, (1 << 31) // NMAX)) == -3                                   # N * plane = 2^31
    assert call(n_s=1, Q=8, Bk=1 << 14, row_len=(0, 1 << 14)) == -3                                     # Q * plane = 2^31
    assert call(G=2, n_s=2, Bk=1 << 15, row_len=(1, 1 << 15)) == -3
    assert call() == 0 and call(src=(1, None), out=(2, None)) == 0 and call(G=4, Q=8, n_s=2) == 0       # groups past G: not looked at
    assert call(Q=1, n_s=1, Bk=4) == 0
    torch.cuda.synchronize()


# ---- the engine ---------------------------------------------------------------------------------------------------------------
def test_shapes_dtypes_and_keys():
    QE.check_shapes(DEV)


def test_open_loop_quantiles_are_the_restatement_on_the_trajectories():
    QE.check_open_loop(DEV)


def test_quantiles_describe_the_prediction_under_observations():
    QE.check_under_observations(DEV)


def test_rows_quantiles():
    QE.check_rows(DEV, exact=False)


def test_order_and_bounds():
    QE.check_order_and_bounds(DEV)


def rows_q_close(a, b, rows):
    """rows_q of two runs within RTOL_SUM x max |rows| of the (step, row) column."""
    return bool(((a.double() - b.double()).abs() <= RTOL_SUM * rows.double().abs().amax(1, keepdim=True)).all())


def test_captured_quantiles_equal_eager_on_one_philox_stream():
    """use_graph=True against an eager engine with the same seed, three calls with new inputs.  One graph, its key ends
    ("samples", N), ("quantiles", (...)); the capture's eager warm-up takes the first T blocks, so replay c is eager call c + 1:
    ``*_q`` the same bits, ``rows_q`` within the bound of what atomics add behind ``rows``."""
    seed = 6
    model = TMM.build(False, DEV)
    av = RC.start()[1]
    xs = [E.dev_list(RC.start(910 + c)[0], DEV) for c in range(3)]
    tgs = [E.dev_list(RC.frames(920 + c), DEV) for c in range(3)]
    obs, otab = E.dev_list(RC.frames(929), DEV), RC.mixed_table(17)
    call = lambda eng, c: E.keep(eng.rollout([xs[c][0], xs[c][1]], pose=xs[c][2], steps=T, available=av, sample=True, samples=N,
                                             quantiles=QE.QS, observed=[None, obs[1], None], observed_available=otab,
                                             targets=tgs[c], **EE.KW))
    eager = MVAEInference(model, seed=seed, use_graph=False)
    e = [call(eager, c) for c in (0, 0, 1, 2)]
    graph = MVAEInference(model, seed=seed)
    assert graph.use_graph
    g = [call(graph, c) for c in range(3)]
    assert len(graph._graphs) == 1
    key = next(iter(graph._graphs))
    assert key[:3] == ("rollout", T, True) and key[-2:] == (("samples", N), ("quantiles", QE.QS))
    for c in range(3):
        a, b = g[c], e[c + 1]
        for k in ("visual_q", "tactile_q", "pose_q") + EE.STATES:
            assert torch.equal(a[k], b[k]), (c, k, float((a[k] - b[k]).abs().max()))
        assert rows_q_close(a["rows_q"], b["rows_q"], b["rows"]), c
    assert not torch.equal(g[0]["visual_q"], g[1]["visual_q"]) and not torch.equal(g[1]["rows_q"], g[2]["rows_q"])
    graph.close(), eager.close()


def test_quantiles_on_dirty_allocator_memory(monkeypatch):
    """Eager, mixed start, observed touch under a table, targets: every torch.empty of ops / layers / engine pre-filled with
    zeros, NaNs or junk (tests/dirty.py), and the real torch.empty: the same bits; the fp64 tables, the rows assembled from them,
    their quantiles and the spread come from atomics (rtol 1e-12)."""
    inputs, av = RC.start()
    inputs, eps = E.dev_list(inputs, DEV), EE.blocks(N, 46)
    obs, tgs, tab = E.dev_list(RC.frames(931), DEV), E.dev_list(RC.frames(932), DEV), RC.mixed_table(18)
    got = {}
    for fill in (None,) + dirty.FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else dirty.PoisonTorch(fill))
        eng = MVAEInference(TMM.build(False, DEV), use_graph=False)
        try:
            r = QE.qroll(eng, inputs, av, eps, N, observed=[None, obs[1], None], observed_available=tab, targets=tgs,
                         target_available=tab, **EE.KW)
            torch.cuda.synchronize()
            got["real torch.empty" if fill is None else fill] = {k: v.detach().cpu().clone() for k, v in r.items()}
        finally:
            eng.close()
    dirty.assert_same_bits(got, approx=E.TERMS + ("spread", "rows_q"), what="ensemble quantiles: ")
