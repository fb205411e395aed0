"""Ensemble rollout on a real MI355X: mmdyn_ensemble_feed -- its ``out`` against mmdyn_rollout_feed on the N * B rows (bit for bit),
with NaN on the observation rows it must not load; its statistics against an fp64 two-pass over the existing kernel's bits of the
prediction; dirty destinations; bad arguments -- then ``MVAEInference.rollout(samples=N)``: the checks of
tests/test_ensemble_emu.py on the HIP library, captured against eager on one Philox stream, and on dirty allocator memory.  The
reference has no rollout: nothing here comes from a golden file."""
import ctypes

import numpy as np
import pytest
import torch

import dirty
import philox_ref as P
import rollout_cases as RC
import test_ensemble_emu as EE
import test_mixed_modal_emu as TMM
import test_rollout_emu as E
from mmdyn_hip import _lib, engine, layers, ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from test_elbo_rows_gpu import RTOL_SUM          # (that file's constant, not a new one)
from test_noise_gpu import NORMAL_TOL
from test_rollout_gpu import gen, table_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
T, B, L, N = EE.T, EE.B, EE.L, EE.N
ATOMIC_RTOL = 1e-12          # fp64 sums that atomics add in any order: the bound tests/dirty.py puts on them


def shifted(rows, n, shift, fill=0.0):
    """[rows, n] fp32 on the device that starts ``shift`` floats past a 16-byte boundary."""
    t = torch.full((rows * n + 4,), fill, device=DEV)[shift:shift + rows * n].view(rows, n)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * shift
    return t


def operands(row_lens, n_s, Bk, seed, shift=0):
    """Per group {recon [N * B, n], obs [B, n], out, mean, var, spread, logits, column} on the device; ``shift``: every out, mean and
    var starts that many floats past a 16-byte boundary.  The pose-sized group (7) and the second 12-float group hold plain signed
    values, the others logits (as tests/test_rollout_gpu.py::operands)."""
    groups = []
    for g, n in enumerate(row_lens):
        groups.append(dict(recon=(3.0 * gen(seed + g, n_s * Bk, n)).to(DEV),
                           obs=torch.rand(Bk, n, generator=torch.Generator().manual_seed(seed + 10 + g)).to(DEV),
                           out=shifted(n_s * Bk, n, shift), mean=shifted(Bk, n, shift), var=shifted(Bk, n, shift),
                           spread=torch.zeros(Bk, dtype=torch.float64, device=DEV), logits=n != 7 and (g, n) != (1, 12),
                           column=(g if n != 7 else 2)))
    return groups


def feed_ref(groups, table, n_s, Bk, observed=True):
    """mmdyn_rollout_feed on the N * B rows, obs and the table repeated N times by the test (``observed=False``: nothing observed --
    the existing kernel's bits of the prediction)."""
    ref = [dict(recon=g["recon"], obs=g["obs"].repeat(n_s, 1) if observed and g["obs"] is not None else None,
                out=torch.full_like(g["recon"], float("nan")), logits=g["logits"], column=g["column"]) for g in groups]
    HIP.rollout_feed(ref, None if table is None else table.repeat(n_s, 1), n_s * Bk)
    return [r["out"] for r in ref]


def clear(groups):
    for g in groups:
        g["out"].fill_(float("nan")), g["mean"].fill_(float("nan")), g["var"].fill_(float("nan")), g["spread"].zero_()


def snapshot(groups):
    return [{k: g[k].clone() for k in ("out", "mean", "var", "spread")} for g in groups]


# the issue's operands: the element path at N = 1; the quad path with the pose on the element path (B * 7 = 35); pose quads that
# straddle rows (B * 7 = 28); N past the unroll factor and odd, more quads than a block, one group unobserved; destinations off
# the 16-byte boundary; the real frame
CASES = [((7,), 1, 1, 0, False, ()), ((48, 48, 7), 3, 5, 0, True, ()), ((48, 48, 7), 2, 4, 0, True, ()),
         ((48, 48, 7), 9, 37, 0, True, (1,)), ((12, 12), 3, 3, 1, True, ()), ((12288, 12288, 7), 4, 2, 0, True, ())]


@pytest.mark.parametrize("row_lens,n_s,Bk,shift,with_table,no_obs", CASES)
def test_out_has_the_bits_of_rollout_feed(row_lens, n_s, Bk, shift, with_table, no_obs):
    """1. ``out`` against mmdyn_rollout_feed on the N * B rows.  With NaN over every obs row that must not be loaded, out, mean and
    var stay finite and keep their bits; without any obs, mean and var keep their bits and spread its value -- to ATOMIC_RTOL:
    the header lets the order of its fp64 atomics differ between runs."""
    groups = operands(row_lens, n_s, Bk, 940 + Bk, shift)
    for g in no_obs:
        groups[g]["obs"] = None
    on, table = table_of(Bk, 950 + Bk) if with_table else (torch.ones(Bk, 3, dtype=torch.bool), None)
    clear(groups)
    HIP.ensemble_feed(groups, table, n_s, Bk)
    for g, w in zip(groups, feed_ref(groups, table, n_s, Bk)):
        assert dirty.first_diff(g["out"], w) is None, (g["column"], dirty.first_diff(g["out"], w))
        assert all(bool(torch.isfinite(g[k]).all()) for k in ("out", "mean", "var", "spread"))
    first = snapshot(groups)
    for g in groups:
        if g["obs"] is not None:
            g["obs"][~on[:, g["column"]].to(DEV)] = float("nan")
    clear(groups)
    HIP.ensemble_feed(groups, table, n_s, Bk)
    for g, c in zip(groups, first):
        for k in ("out", "mean", "var"):
            assert dirty.first_diff(g[k], c[k]) is None and bool(torch.isfinite(g[k]).all()), (g["column"], k)
        assert torch.allclose(g["spread"], c["spread"], rtol=ATOMIC_RTOL, atol=0.0)
    for g in groups:
        g["obs"] = None
    clear(groups)
    HIP.ensemble_feed(groups, table, n_s, Bk)
    for g, c, p in zip(groups, first, feed_ref(groups, table, n_s, Bk, observed=False)):
        assert dirty.first_diff(g["out"], p) is None
        for k in ("mean", "var"):
            assert dirty.first_diff(g[k], c[k]) is None, (g["column"], k)
        assert torch.allclose(g["spread"], c["spread"], rtol=ATOMIC_RTOL, atol=0.0)


@pytest.mark.parametrize("row_lens,n_s,Bk,shift,with_table,no_obs", CASES)
def test_statistics(row_lens, n_s, Bk, shift, with_table, no_obs):
    """2. mean, var and spread against an fp64 two-pass over p, taken from mmdyn_rollout_feed's unobserved output (the existing
    kernel's bits of the sigmoid), under the derived bounds of tests/test_ensemble_emu.py::assert_stats; N identical samples give
    var == 0 and mean == p exactly."""
    groups = operands(row_lens, n_s, Bk, 960 + Bk, shift)
    for g in no_obs:
        groups[g]["obs"] = None
    _, table = table_of(Bk, 970 + Bk) if with_table else (None, None)
    clear(groups)
    HIP.ensemble_feed(groups, table, n_s, Bk)
    for g, p in zip(groups, feed_ref(groups, table, n_s, Bk, observed=False)):
        EE.assert_stats(g["mean"].cpu(), g["var"].cpu(), g["spread"].cpu(), p.view((n_s, Bk) + tuple(p.shape[1:])).cpu(),
                        f"group {g['column']}")
        if n_s > 1:
            assert float(g["var"].max()) > 0.0
    for g in groups:
        g["recon"].copy_(g["recon"][:Bk].repeat(n_s, 1))
    clear(groups)
    HIP.ensemble_feed(groups, table, n_s, Bk)
    for g, p in zip(groups, feed_ref(groups, table, n_s, Bk, observed=False)):
        assert float(g["var"].abs().max()) == 0.0 and float(g["spread"].abs().max()) == 0.0
        assert dirty.first_diff(g["mean"], p[:Bk]) is None


def test_a_nan_sample_stays_in_its_element():
    """2. A NaN in recon[n][b] of one group reaches out[n][b] and the mean / var / spread of row b in that group at that element;
    everything else keeps its bits (spread: ATOMIC_RTOL)."""
    row_lens, n_s, Bk = (48, 48, 7), 3, 5
    groups = operands(row_lens, n_s, Bk, 980)
    on, table = table_of(Bk, 981)
    assert not bool(on[1].any())                                    # row 1 takes no observation
    clear(groups)
    HIP.ensemble_feed(groups, table, n_s, Bk)
    first = snapshot(groups)
    n, b, i = 1, 1, 5
    groups[0]["recon"][n * Bk + b, i] = float("nan")
    clear(groups)
    HIP.ensemble_feed(groups, table, n_s, Bk)
    for gi, (g, c) in enumerate(zip(groups, first)):
        hit = {k: torch.zeros_like(g[k], dtype=torch.bool) for k in ("out", "mean", "var", "spread")}
        if gi == 0:
            hit["out"][n * Bk + b, i] = hit["mean"][b, i] = hit["var"][b, i] = hit["spread"][b] = True
        for k in ("out", "mean", "var", "spread"):
            assert bool(torch.isnan(g[k][hit[k]]).all()) and not bool(torch.isnan(g[k][~hit[k]]).any()), (gi, k)
            if k == "spread":
                assert torch.allclose(g[k][~hit[k]], c[k][~hit[k]], rtol=ATOMIC_RTOL, atol=0.0)
            else:
                assert dirty.first_diff(g[k][~hit[k]], c[k][~hit[k]]) is None, (gi, k)


def test_feed_on_dirty_destinations():
    """3. Zero-, NaN- and junk-filled out, mean and var (tests/dirty.py): the same bits; the inputs and the table are not written;
    spread is an accumulator with a documented initial value (state, ATOMIC_RTOL)."""
    row_lens, n_s, Bk = (48, 48, 7), 3, 5
    src = operands(row_lens, n_s, Bk, 990)
    _, table = table_of(Bk, 991)

    def feed(backend, recon, obs, out, mean, var, spread, tab):
        backend.ensemble_feed([dict(recon=r, obs=o, out=d, mean=m, var=v, spread=s, logits=g["logits"], column=g["column"])
                               for r, o, d, m, v, s, g in zip(recon, obs, out, mean, var, spread, src)], tab, n_s, Bk)
    args = ([g["recon"] for g in src], [g["obs"] for g in src], [torch.empty(n_s * Bk, n) for n in row_lens],
            [torch.empty(Bk, n) for n in row_lens], [torch.empty(Bk, n) for n in row_lens],
            [torch.zeros(Bk, dtype=torch.float64) for _ in row_lens], table)
    runs = dirty.run_dirty(HIP, feed, args, outs=[2, 3, 4], state=[5], device=DEV)
    dirty.assert_same_bits(runs, approx=[f"spread[{g}]" for g in range(3)], rtol=ATOMIC_RTOL, what="ensemble_feed: ")


def test_feed_rejects_bad_arguments():
    """4. MMDYN_ERR_NULL / _SHAPE / _RANGE from the raw entry point, before any launch."""
    lib, t = HIP.lib, torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    # per group (stride 1024 bytes), N = B = 2 and rows of 4 floats: recon [4][4] at +0, obs [2][4] at +64, out at +128, mean at +192,
    # var at +224, spread [2] at +256

    def call(G=1, n_s=2, Bk=2, table=None, **over):
        a = _lib.EnsembleGroups()
        for g in range(4):
            q = p + 1024 * g
            a.recon[g], a.obs[g], a.out[g], a.mean[g], a.var[g], a.spread[g] = q, q + 64, q + 128, q + 192, q + 224, q + 256
            a.row_len[g], a.logits[g], a.column[g] = 4, 0, g
        for k, (g, v) in over.items():
            getattr(a, k)[g] = v
        return lib.mmdyn_ensemble_feed(ctypes.addressof(a), G, table, n_s, Bk, None)
    assert lib.mmdyn_ensemble_feed(None, 1, None, 1, 1, None) == -2
    assert call(recon=(0, None)) == -2 and call(out=(0, None)) == -2 and call(mean=(0, None)) == -2 and call(G=2, out=(1, None)) == -2
    assert call(G=0) == -1 and call(G=5) == -1 and call(n_s=0) == -1 and call(Bk=0) == -1
    assert call(row_len=(0, 0)) == -1 and call(column=(0, 4)) == -1 and call(column=(0, -1)) == -1
    assert call(table=p + 2048 + 1) == -1                                       # misaligned table
    assert call(var=(0, None)) == -1                                            # spread without var
    assert call(out=(0, p)) == -1 and call(out=(0, p + 64 + 8)) == -1           # out overlaps recon / obs
    assert call(mean=(0, p + 60)) == -1 and call(var=(0, p + 32)) == -1 and call(spread=(0, p + 64)) == -1
    assert call(mean=(0, p + 128 + 32)) == -1 and call(var=(0, p + 192 + 4)) == -1 and call(spread=(0, p + 192)) == -1   # two outputs
    assert call(G=2, out=(1, p)) == -1 and call(G=2, mean=(1, p + 64)) == -1    # an output on another group's inputs
    assert call(G=2, var=(1, p + 128)) == -1                                    # ... and on another group's output
    assert call(table=p + 128) == -1 and call(table=p + 256) == -1              # an output on the table
    assert call(n_s=32768, Bk=1, row_len=(0, 65536)) == -3                      # N * B * row_len = 2^31
    assert call(n_s=2, Bk=32768, row_len=(0, 32768)) == -3
    assert call(G=2, n_s=16384, Bk=2, row_len=(1, 65536)) == -3
    assert call(recon=(1, None)) == 0 and call(G=4, table=p + 3072 + 512) == 0  # groups past G are not looked at
    assert call(obs=(0, None), var=(0, None), spread=(0, None)) == 0
    torch.cuda.synchronize()


# ---- the engine ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    """What fp64 atomics add up behind the decoders: the bound tests/test_rollout_gpu.py puts on such sums."""
    if a is None or b is None:
        return a is None and b is None
    return torch.allclose(a.double(), b.double(), rtol=RTOL_SUM, atol=0.0)


def test_one_sample_is_todays_rollout():
    EE.check_one_sample_is_todays_rollout(DEV, same)


def test_every_trajectory_is_todays_rollout_on_its_draws():
    EE.check_every_trajectory(DEV)


def test_engine_statistics():
    EE.check_statistics(DEV)


def test_conditions():
    EE.check_conditions(DEV)


def philox_blocks(seed, first, n):
    """The T draws of one ensemble call from the exact reference, rounded to fp32: step t sits at counter first + t * n."""
    return [torch.from_numpy(P.normal_ref(N * B * L, seed, first + t * n)[0].astype(np.float32)).reshape(N * B, L) for t in range(T)]


EXACT = ("means", "log_var") + EE.STATES + EE.STATS      # written once by one thread each: the same bits in every run


def test_captured_ensemble_equals_eager_on_one_philox_stream():
    """6. use_graph=True against an eager engine with the same seed, three calls with new inputs.  One graph, its key carries N;
    the capture's eager warm-up takes the first T blocks, so replay c is eager call c + 1: the same bits wherever one thread
    writes an element once, RTOL_SUM for what atomics add (the tables, the rows assembled from them, the spread).  The draws:
    step t of eager call k draws at counter (k T + t) n with n = counters_of(N B L); a rollout with the reference's numbers INJECTED
    at those counters gives the engine's means to OUT_TOL (a device normal is within NORMAL_TOL of the reference), the next call's
    counters give means further away than 100 x the tolerance."""
    seed, n = 5, P.counters_of(N * B * L)
    assert NORMAL_TOL < 1e-4
    model = TMM.build(False, DEV)
    av = RC.start()[1]
    xs = [E.dev_list(RC.start(880 + c)[0], DEV) for c in range(3)]
    tgs = [E.dev_list(RC.frames(890 + c), DEV) for c in range(3)]
    obs, otab = E.dev_list(RC.frames(899), DEV), RC.mixed_table(13)
    call = lambda eng, c: E.keep(eng.rollout([xs[c][0], xs[c][1]], pose=xs[c][2], steps=T, available=av, sample=True, samples=N,
                                             observed=[None, obs[1], None], observed_available=otab, targets=tgs[c], **EE.KW))
    eager = MVAEInference(model, seed=seed, use_graph=False)
    e = [call(eager, c) for c in (0, 0, 1, 2)]
    graph = MVAEInference(model, seed=seed)
    assert graph.use_graph
    g = [call(graph, c) for c in range(3)]
    assert len(graph._graphs) == 1
    key = next(iter(graph._graphs))
    assert key[:3] == ("rollout", T, True) and key[-1] == ("samples", N)
    for c in range(3):
        a, b = g[c], e[c + 1]
        for k in EXACT:
            assert torch.equal(a[k], b[k]), (c, k, float((a[k] - b[k]).abs().max()))
        for k in E.TERMS + ("spread",):
            assert same(a[k], b[k]), (c, k)
    assert not torch.equal(g[0]["means"], g[1]["means"]) and not torch.equal(g[1]["visual_var"], g[2]["visual_var"])
    inj = MVAEInference(model, use_graph=False)
    tol = TMM.OUT_TOL
    for who, res, first, inputs in (("eager", e, 0, (0, 0, 1, 2)), ("graph", g, 1, (0, 1, 2))):
        for c, r in enumerate(res):
            for block, near in ((c + first, True), (c + first + 1, False)):
                x = xs[inputs[c]]
                m = EE.eroll(inj, x, av, philox_blocks(seed, block * T * n, n), N, observed=[None, obs[1], None],
                             observed_available=otab)["means"]
                d = (m - r["means"]).abs()
                print(who, "call", c, "draws of block", block, "largest / median |means - injected|", float(d.max()), float(d[1:].median()))
                if near:
                    np.testing.assert_allclose(m.cpu().numpy(), r["means"].cpu().numpy(), **tol, err_msg=f"{who} {c}")
                else:
                    assert float(d[1:].median()) > 100 * tol["atol"], (who, c)
    graph.close(), eager.close(), inj.close()


def test_ensemble_on_dirty_allocator_memory(monkeypatch):
    """6. Eager, mixed start, observed touch under a table, targets: every torch.empty of ops / layers / engine pre-filled with
    zeros, NaNs or junk (tests/dirty.py), and the real torch.empty: the same bits; the fp64 tables, the rows assembled from them
    and the spread come from atomics (rtol 1e-12)."""
    inputs, av = RC.start()
    inputs, eps = E.dev_list(inputs, DEV), EE.blocks(N, 38)
    obs, tgs, tab = E.dev_list(RC.frames(863), DEV), E.dev_list(RC.frames(864), DEV), RC.mixed_table(14)
    got = {}
    for fill in (None,) + dirty.FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else dirty.PoisonTorch(fill))
        eng = MVAEInference(TMM.build(False, DEV), use_graph=False)
        try:
            r = EE.eroll(eng, inputs, av, eps, N, observed=[None, obs[1], None], observed_available=tab, targets=tgs,
                         target_available=tab, **EE.KW)
            torch.cuda.synchronize()
            got["real torch.empty" if fill is None else fill] = {k: v.detach().cpu().clone() for k, v in r.items()}
        finally:
            eng.close()
    dirty.assert_same_bits(got, approx=E.TERMS + ("spread",), what="ensemble rollout: ")
