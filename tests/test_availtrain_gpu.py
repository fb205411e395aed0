"""The fused training step on mixed-modality batches on a real MI355X: the three new entry points (mmdyn_poe_bwd_avail_weighted,
mmdyn_term_weights, mmdyn_elbo_assemble_avail_weighted) element by element against fp64 torch restatements and bit for bit against
their siblings, with guard bands and pre-filled outputs; MVAEStep against the yardstick of tests/availtrain_cases.py; all-ones tables
against the plain step; graph replay with changing tables.

Kernel-level batch sizes: 1 (one row), 5 (odd), 257 (past one 256-thread block).  L = 32 puts two rows into one wavefront (the
per-expert branch diverges inside it), L = 256 keeps a wavefront inside a row."""
import ctypes

import pytest
import torch

import availtrain_cases as A
import test_availtrain_emu as TA
import test_model_emu as T
from dirty import JUNK, NAN, ZERO, bits, fill_
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models.vae import NoiseSource
from mmdyn_hip.utils.seeded_init import seeded_batch
from test_kernels_aten_gpu import rel, rnd
from test_weighted_gpu import guarded, guards_intact, f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
SUBSETS = [(1, 1, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1)]
BATCHES = [1, 5, 257]


def stream():
    return torch.cuda.current_stream().cuda_stream


def pattern(B, shift):
    """uint8 [B][4]: row b holds the subset whose bits are (b + shift) % 8 -- every pattern, the empty one included."""
    code = (torch.arange(B) + shift) % 8
    return torch.stack([(code >> m) & 1 for m in range(3)] + [torch.zeros(B, dtype=torch.long)], 1).to(torch.uint8).to(DEV)


def weights(B, seed=3):
    """Mixed magnitudes, a zero and a negative weight (B permitting)."""
    w = A.weights(B, seed)
    if B > 2:
        w[1], w[2] = 0.0, -0.75
    return w.to(DEV)


# ---- mmdyn_poe_bwd_avail_weighted --------------------------------------------------------------------------------------------------
def poe_problem(B, L, seed):
    P = len(SUBSETS)
    heads = [(rnd(B, 2 * L, seed=seed + m) * 0.7).to(DEV) for m in range(3)]
    eps = rnd(P, B, L, seed=seed + 9).to(DEV)
    dzs = [[(rnd(B, L, seed=seed + 20 + 3 * p + k) * 0.1).to(DEV) if s[k] else None for k in range(3)] for p, s in enumerate(SUBSETS)]

    def passes(dheads=None):
        out = []
        for p, s in enumerate(SUBSETS):
            hs = [heads[m] if s[m] else None for m in range(3)]
            ds = [dheads[p][m] if (dheads is not None and s[m]) else None for m in range(3)]
            out.append({"mu": [None if h is None else h[:, :L] for h in hs], "lv": [None if h is None else h[:, L:] for h in hs],
                        "dmu": [None if d is None else d[:, :L] for d in ds], "dlv": [None if d is None else d[:, L:] for d in ds],
                        "ld": [2 * L] * 3, "dz": dzs[p]})
        return out
    return heads, eps, dzs, passes


@pytest.mark.parametrize("L", [32, 256])
@pytest.mark.parametrize("B", BATCHES)
def test_poe_bwd_avail_weighted(B, L):
    P, ks, klw_v = len(SUBSETS), 0.013, 0.6
    heads, eps, dzs, passes = poe_problem(B, L, 900 + B + L)
    klw = torch.tensor([klw_v], device=DEV)
    tab = pattern(B, 3)
    on = tab[:, :3] != 0

    def forward(table):
        mu, lv = torch.empty(P, B, L, device=DEV), torch.empty(P, B, L, device=DEV)
        HIP.poe_fwd_avail(passes(), None if table is None else [table] * P, eps, mu, lv, torch.empty(P, B, L, device=DEV), None, True,
                          P, B, L)
        return mu, lv

    def run(kind, fw, table=None, w=None, fill=12345.0):
        bufs = [[guarded(B * 2 * L) for _ in range(3)] for _ in range(P)]
        for row in bufs:
            for b in row:
                b[1].fill_(fill)
        dh = [[b[1].view(B, 2 * L) for b in row] for row in bufs]
        tabs = None if table is None else [table] * P
        if kind == "avail":
            HIP.poe_bwd_avail(passes(dh), tabs, eps, fw[0], fw[1], None, None, None, ks, True, P, B, L, klw)
        elif kind == "weighted":
            HIP.poe_bwd_weighted(passes(dh), eps, fw[0], fw[1], None, None, None, ks, w, True, P, B, L, klw)
        else:
            HIP.poe_bwd_avail_weighted(passes(dh), tabs, eps, fw[0], fw[1], None, None, None, ks, w, True, P, B, L, klw)
        torch.cuda.synchronize()
        assert all(guards_intact(b[0]) for row in bufs for b in row)
        return [[dh[p][m] if SUBSETS[p][m] else None for m in range(3)] for p in range(P)]

    def same(a, b):
        return all(torch.equal(a[p][m], b[p][m]) for p in range(P) for m in range(3) if SUBSETS[p][m])

    fw_tab, fw_all = forward(tab), forward(None)
    ones, w = torch.ones(B, device=DEV), weights(B)
    # the siblings, bit for bit: w = 1 -> mmdyn_poe_bwd_avail; a null table (no array, or null entries) -> mmdyn_poe_bwd_weighted
    assert same(run("both", fw_tab, tab, ones), run("avail", fw_tab, tab))
    assert same(run("both", fw_all, None, w), run("weighted", fw_all, None, w))
    got = run("both", fw_tab, tab, w)
    assert same(got, run("both", fw_tab, tab, w, fill=float("nan")))           # whatever the buffers held
    # fp64 autograd on each row's own expert set, the KL of row b scaled by ks * klw * w_b.  Bound: the criterion of
    # test_poe_bwd_weighted (1e-4 relative L2 per tensor: ~30 fp32 operations per element, expf among them, with cancellation between
    # the dS terms), and element by element 1e-4 of the tensor's largest magnitude
    eps_p = 1e-8
    for p, s in enumerate(SUBSETS):
        hs = [heads[m].double().clone().requires_grad_(True) if s[m] else None for m in range(3)]
        sumT = torch.ones(B, L, dtype=torch.float64, device=DEV) / (1.0 + 2 * eps_p)
        sumMuT = torch.zeros(B, L, dtype=torch.float64, device=DEV)
        for m, h in enumerate(hs):
            if h is not None:
                T_ = 1.0 / (torch.exp(h[:, L:]) + 2 * eps_p)
                row = on[:, m:m + 1]
                sumT, sumMuT = torch.where(row, sumT + T_, sumT), torch.where(row, sumMuT + h[:, :L] * T_, sumMuT)
        pm, plv = sumMuT / sumT, torch.log(1.0 / sumT + eps_p)
        for a, b in ((fw_tab[0][p], pm.detach()), (fw_tab[1][p], plv.detach())):   # (a row without experts: mu = 0, lv ~ 3e-8)
            assert float((a.double() - b).abs().max()) <= 1e-5 * (1.0 + float(b.abs().max()))
        obj = ((ks * klw_v * w.double())[:, None] * (-0.5 * (1 + plv - pm * pm - plv.exp()))).sum()
        gz = sum(t.double() for t in dzs[p] if t is not None)
        obj = obj + ((eps[p].double() * torch.exp(0.5 * plv) + pm) * gz).sum()
        obj.backward()
        for m in range(3):
            if s[m]:
                want = hs[m].grad
                assert rel(got[p][m], want) < 1e-4, (p, m, rel(got[p][m], want))
                err = (got[p][m].double() - want).abs()
                assert float(err.max()) <= 1e-4 * float(want.abs().max()), (p, m)
                absent = ~on[:, m]
                assert float(got[p][m][absent].abs().sum()) == 0.0 and float(want[absent].abs().sum()) == 0.0
    # arguments
    lib = HIP.lib
    assert lib.mmdyn_poe_bwd_avail_weighted(None, None, None, None, None, None, None, None, 1.0, None, 1, 1, 1, 1, None, None) == -2
    dh = [[torch.zeros(B, 2 * L, device=DEV) for _ in range(3)] for _ in range(P)]
    arr = ctypes.cast(HIP._passes(passes(dh)), ctypes.c_void_p)
    raw = torch.ones(B * 4 + 4, dtype=torch.uint8, device=DEV)
    call = lambda t, wk, prior=1, PP=P: lib.mmdyn_poe_bwd_avail_weighted(
        arr, ctypes.addressof(t), eps.data_ptr(), fw_tab[0].data_ptr(), fw_tab[1].data_ptr(), None, None, None, ks, wk, prior, PP, B, L,
        None, stream())
    good = (ctypes.c_void_p * 8)(*[raw.data_ptr()] * P)
    odd = (ctypes.c_void_p * 8)(*[raw.data_ptr() + 1] * P)
    assert call(good, None) == -2                      # the weights are required
    assert call(odd, w.data_ptr()) == -1               # a table off the 4-byte grid
    assert call(good, w.data_ptr(), prior=0) == -1     # a table without the prior
    assert call(good, w.data_ptr(), PP=9) == -1
    torch.cuda.synchronize()
    assert all(float(d.abs().sum()) == 0.0 for row in dh for d in row)         # nothing was launched
    with pytest.raises(ValueError):
        HIP.poe_bwd_avail_weighted(passes(dh), [tab] * P, eps, fw_tab[0], fw_tab[1], None, None, None, ks, torch.ones(B + 1, device=DEV),
                                   True, P, B, L, klw)


# ---- mmdyn_term_weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_term_weights(B):
    tab = pattern(B, 1)
    on = (tab[:, :3] != 0).t()                        # [3][B]
    w = weights(B)
    zero = torch.zeros(B, device=DEV)
    for ww, table in ((w, tab), (None, tab), (w, None), (None, None)):
        runs = []
        for fill in (ZERO, NAN, JUNK, ZERO):
            buf, out = guarded(3 * B)
            fill_(out, fill)
            HIP.term_weights(table, ww, out.view(3, B), B)
            torch.cuda.synchronize()
            assert guards_intact(buf)
            runs.append(out.clone())
        assert all(torch.equal(bits(r), bits(runs[0])) for r in runs)          # whatever the buffer held; run to run
        base = torch.ones(B, device=DEV) if ww is None else ww
        want = base.expand(3, B) if table is None else torch.where(on, base.expand(3, B), zero.expand(3, B))
        assert torch.equal(runs[0].view(3, B), want)                           # element by element: a selection is exact
    # a NaN / Inf weight of an absent (row, term) reaches nothing: selected, never multiplied
    bad = w.clone()
    bad[0] = float("nan")
    t0 = tab.clone()
    t0[0, :3] = 0
    out = torch.empty(3, B, device=DEV)
    HIP.term_weights(t0, bad, out, B)
    assert float(out[:, 0].abs().sum()) == 0.0 and bool(torch.isfinite(out).all())
    lib = HIP.lib
    raw = torch.ones(B * 4 + 4, dtype=torch.uint8, device=DEV)
    keep = out.clone()
    assert lib.mmdyn_term_weights(raw.data_ptr(), None, None, B, stream()) == -2
    assert lib.mmdyn_term_weights(raw.data_ptr() + 1, None, out.data_ptr(), B, stream()) == -1
    assert lib.mmdyn_term_weights(raw.data_ptr(), None, out.data_ptr(), 0, stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
    with pytest.raises(ValueError):
        HIP.term_weights(tab, w, torch.empty(3, B + 1, device=DEV), B)
    with pytest.raises(ValueError):
        HIP.term_weights(tab[:, :3], w, out, B)


# ---- mmdyn_elbo_assemble_avail_weighted -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_elbo_assemble_avail_weighted(B):
    P, pm, klw_arg, klw_dev = 7, 1000.0, 0.5, 0.04
    gen = torch.Generator().manual_seed(940 + B)
    bv = (torch.rand(P, B, dtype=torch.float64, generator=gen) * 9000).to(DEV)
    bt = (torch.rand(P, B, dtype=torch.float64, generator=gen) * 7000).to(DEV)
    mse = torch.rand(P, B, dtype=torch.float64, generator=gen).to(DEV)
    klr = (torch.rand(P, B, dtype=torch.float64, generator=gen) * 40).to(DEV)
    kls = klr.sum(1)
    kd = torch.tensor([klw_dev], device=DEV)
    tab = pattern(B, 2)
    on = (tab[:, :3] != 0).t()                        # [3][B]
    w = weights(B)

    def run(tables, ww, table, mode, fill=ZERO):
        tv, tt, tm = (None if t is None else t.clone() for t in tables)
        lbuf, loss = guarded(1)
        pbuf, wp = guarded(P)
        obuf, out = guarded(B)
        qbuf, parts = guarded(P * B)
        sbuf, ws = guarded(B)
        pres, sums = f64(3), f64(3, P)
        for t in (loss, wp, out, parts, ws, pres, sums):
            fill_(t, fill)
        HIP.elbo_assemble_avail_weighted(tv, tt, tm, klr, kls, ww, table, loss, wp, out, parts, ws, pres, sums, P, B, klw_arg, pm, kd,
                                         mode)
        torch.cuda.synchronize()
        assert all(guards_intact(b) for b in (lbuf, pbuf, obuf, qbuf, sbuf))
        return dict(loss=loss.clone(), wp=wp.clone(), out=out.clone(), parts=parts.clone(), ws=ws.clone(), pres=pres, sums=sums,
                    tv=tv, tt=tt, tm=tm)

    def same(a, b):
        return all((a[k] is None and b[k] is None) or torch.equal(bits(a[k]), bits(b[k])) for k in a)

    for mode in (0, 1):
        for ww in (w, None):
            got = run((bv, bt, mse), ww, tab, mode)
            # whatever the output buffers held, and run to run: the same bits
            assert same(got, run((bv, bt, mse), ww, tab, mode, NAN)) and same(got, run((bv, bt, mse), ww, tab, mode, JUNK))
            assert same(got, run((bv, bt, mse), ww, tab, mode))
            # fp64 torch, element by element.  Bounds: out / partials / wpartials / loss are fp32 roundings of fp64 sums of
            # non-negative-magnitude terms added in another order (rtol 1e-6 >> 2^-24, atol for cancelling negative weights);
            # term_sums are fp64 sums in another order (1e-12); the counts and the written-back tables are exact
            wd = torch.ones(B, dtype=torch.float64, device=DEV) if ww is None else ww.double()
            sel = [torch.where(on[m][None, :], t, torch.zeros_like(t)) for m, t in enumerate((bv, bt, mse))]
            rec = (sel[0] + sel[1]) + pm * sel[2]
            kl_rows = klr if mode else kls[:, None].expand(P, B)
            per = rec + klw_arg * klw_dev * kl_rows
            assert torch.allclose(got["parts"].view(P, B).double(), per, rtol=1e-6, atol=0)
            assert torch.allclose(got["out"].double(), per.sum(0), rtol=1e-6, atol=0)
            kl = (klr * wd).sum(1) if mode else wd.sum() * kls
            want = ((rec * wd).sum(1) + klw_arg * klw_dev * kl) / B
            scale = float(((rec.abs() * wd.abs()).sum(1) / B).max())
            assert torch.allclose(got["wp"].double(), want, rtol=1e-6, atol=1e-6 * scale)
            assert float(got["loss"]) == pytest.approx(float(want.sum()), rel=1e-6, abs=1e-6 * scale * P)
            assert torch.allclose(got["ws"].double(), torch.full((B,), float(wd.sum()), dtype=torch.float64, device=DEV), rtol=1e-6)
            assert len(set(got["ws"].tolist())) == 1
            assert torch.equal(got["pres"], on.double().sum(1))
            assert torch.allclose(got["sums"], torch.stack([s.sum(1) for s in sel]), rtol=1e-12, atol=0)
            for k, s in zip(("tv", "tt", "tm"), sel):
                assert torch.equal(got[k], s)            # absent entries overwritten with 0, present ones untouched
            # NaN / Inf in the entries of absent targets: selected out, the same bits
            dirty = []
            for m, t in enumerate((bv, bt, mse)):
                d = t.clone()
                d[:, ~on[m]] = float("nan") if m != 1 else float("inf")
                dirty.append(d)
            assert same(got, run(dirty, ww, tab, mode))
            # null tables: a term that is not there
            part = run((bv, None, None), ww, tab, mode)
            assert torch.allclose(part["out"].double(), (sel[0] + klw_arg * klw_dev * kl_rows).sum(0), rtol=1e-6, atol=0)
            assert float(part["sums"][1:].abs().sum()) == 0.0 and torch.equal(part["pres"], got["pres"])
        # a null table with w: the bits of mmdyn_elbo_assemble_weighted on the summed tables
        free = run((bv, bt, mse), w, None, mode)
        loss0, wp0, out0, parts0, ws0 = (torch.empty(n, device=DEV) for n in (1, P, B, P * B, B))
        HIP.elbo_assemble_weighted(bv + bt, mse, klr, kls, w, loss0, wp0, out0, parts0, ws0, P, B, klw_arg, pm, kd, mode)
        for k, t in (("loss", loss0), ("wp", wp0), ("out", out0), ("parts", parts0), ("ws", ws0)):
            assert torch.equal(bits(free[k]), bits(t)), k
        assert torch.equal(free["pres"], torch.full((3,), float(B), dtype=torch.float64, device=DEV))
        assert torch.equal(free["tv"], bv) and torch.equal(free["tt"], bt) and torch.equal(free["tm"], mse)
    # arguments
    lib = HIP.lib
    raw = torch.ones(B * 4 + 4, dtype=torch.uint8, device=DEV)
    lw = torch.full((1,), 7.0, device=DEV)
    call = lambda tv, tt, table, loss, PP=P, mode=0: lib.mmdyn_elbo_assemble_avail_weighted(
        tv, tt, None, None, None, None, table, loss, None, None, None, None, None, None, PP, B, 1.0, 1.0, None, mode, stream())
    assert call(None, None, None, None) == -2
    assert call(None, None, raw.data_ptr() + 2, lw.data_ptr()) == -1
    assert call(None, None, raw.data_ptr(), lw.data_ptr(), PP=9) == -1
    assert call(None, None, raw.data_ptr(), lw.data_ptr(), mode=2) == -1
    assert call(bv.data_ptr(), bv.data_ptr(), raw.data_ptr(), lw.data_ptr()) == -1       # one table per term
    torch.cuda.synchronize()
    assert float(lw) == 7.0
    with pytest.raises(ValueError):
        HIP.elbo_assemble_avail_weighted(bv, bt, mse, klr, kls, w, tab, lw, None, torch.empty(B - 1, device=DEV), None, None, None,
                                         None, P, B, 1.0, 1.0)


# ---- the engine -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kl,weighted", [("batch", True), ("sample", True), ("sample", False)])
@pytest.mark.parametrize("name,precision", [("pose", "fp32"), ("nopose", "fp32x3")])
def test_engine_vs_yardstick(name, precision, kl, weighted):
    """The pose case on the native fp32 matrix cores, the case without pose in fp32x3: the split tests/test_weighted_gpu.py uses to
    stay clear of the pose decoder's ReLU knife edges."""
    TA.check_engine_vs_yardstick(DEV, name, kl, weighted, precision)


@pytest.mark.parametrize("which,column", [("target", 1), ("input", 0)])
def test_zero_column_gives_exact_zero_gradients(which, column):
    TA.check_zero_column(DEV, "pose", column, which, "fp32")


def _one_step(precision, B, tables, seed=11):
    inputs, targets = seeded_batch(B, 5)
    gi, gt = [x.to(DEV) for x in inputs], [x.to(DEV) for x in targets]
    m = T.build("cnn-mvae", True, True, DEV)
    step = MVAEStep(m, noise=NoiseSource(seed), precision=precision)
    kw = {} if tables is None else dict(available=tables, target_available=tables, kl="sample")
    loss = float(step.train_step(gi, gt, 0.02, **kw))
    flat = step.params.flat.clone()
    step.close()
    return loss, flat


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_all_ones_tables_equal_the_plain_step(precision):
    """Parameters after one optimiser step with all-ones tables (kl="sample") against the plain step on the same Philox noise, under
    the rule of tests/test_weighted_gpu.py::test_ones_equals_unweighted_step: two plain eager steps are compared first -- bitwise
    repeatable: bitwise equality is demanded; otherwise four times the measured run-to-run difference."""
    B = 37
    l0, p0 = _one_step(precision, B, None)
    l0b, p0b = _one_step(precision, B, None)
    l1, p1 = _one_step(precision, B, torch.ones(B, 3, device=DEV))
    run_to_run = float((p0 - p0b).double().norm() / p0.double().norm())
    diff = float((p1 - p0).double().norm() / p0.double().norm())
    print(f"[{precision}] plain run-to-run {run_to_run:.3e} (bitwise: {torch.equal(p0, p0b)}); all-ones tables against plain {diff:.3e} "
          f"(bitwise: {torch.equal(p1, p0)}); losses {l0!r} {l0b!r} {l1!r}")
    if torch.equal(p0, p0b):
        assert torch.equal(p1, p0)
    else:
        assert diff <= 4 * run_to_run
    assert l1 == pytest.approx(l0, rel=1e-4)


def test_graph_replay_with_changing_tables():
    """Three graphed steps with three different table contents on one engine against three eager steps on a twin engine (the same
    seeded weights and Philox stream): losses to 1e-4, the parameters after the three Adam steps to 1e-3 relative L2; ONE capture
    serves the three mixtures."""
    B, klw = 8, 0.02
    inputs, targets = seeded_batch(B, 5)
    gi, gt = [x.to(DEV) for x in inputs], [x.to(DEV) for x in targets]
    tables = [(pattern(B, s)[:, :3].float(), pattern(B, s + 3)[:, :3].float()) for s in (0, 1, 5)]
    assert not torch.equal(tables[0][0], tables[1][0]) and not torch.equal(tables[1][0], tables[2][0])
    res = []
    for graphed in (False, True):
        m = T.build("cnn-mvae", True, True, DEV)
        step = MVAEStep(m, noise=NoiseSource(11))
        captures = []
        real = step._capture
        step._capture = lambda *a, **k: (captures.append(1), real(*a, **k))[1]
        fn = step.train_step_graphed if graphed else step.train_step
        losses, rows = [], []
        for tin, ttg in tables:
            losses.append(float(fn(gi, gt, klw, kl="sample", available=tin, target_available=ttg)))
            rows.append(step.last_rows["rows"].clone())
            assert torch.equal(step.last_rows["present"].cpu(), (ttg != 0).double().sum(0).cpu())
        res.append((losses, rows, step.params.flat.clone()))
        if graphed:
            assert len(captures) == 1 and step._graph is not None and step._graph[0][-1][0] == "avail"
        step.close()
    print("eager", res[0][0], "graphed", res[1][0])
    assert res[1][0] == pytest.approx(res[0][0], rel=1e-4)
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.allclose(a, b, rtol=1e-4)
    assert TA.rel_l2(res[1][2], res[0][2]) < 1e-3
    assert len(set(res[1][0])) == 3
