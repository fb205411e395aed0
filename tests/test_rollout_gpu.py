"""Multi-step rollout on a real MI355X: mmdyn_rollout_feed against mmdyn_complete_select group by group (bit for bit), with NaN on
the sides it must not load, on dirty destinations and with bad arguments; then ``MVAEInference.rollout`` -- the checks of
tests/test_rollout_emu.py on the HIP library, captured against eager on one Philox stream, and on dirty allocator memory -- and
``DynModeling.rollout``.  The reference has no rollout: nothing here comes from a golden file."""
import ctypes

import numpy as np
import pytest
import torch

import dirty
import philox_ref as P
import rollout_cases as RC
import test_mixed_modal_emu as TMM
import test_rollout_emu as E
from mmdyn_hip import _lib, engine, layers, ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.models.functional import availability_table
from test_elbo_rows_gpu import RTOL_SUM          # (that file's constant, not a new one)
from test_noise_gpu import NORMAL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
T, B, L = E.T, E.B, E.L


def gen(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def operands(Bk, row_lens, seed, shift=0):
    """Per group (recon, obs, out, logits, column) on the device; ``shift``: every out starts that many floats past a 16-byte
    boundary (the element-wise path).  The pose-sized group (7) and the second 12-float group hold plain values, the others logits."""
    groups = []
    for g, n in enumerate(row_lens):
        out = torch.zeros(Bk * n + 4, device=DEV)[shift:shift + Bk * n].view(Bk, n)
        assert out.is_contiguous() and out.data_ptr() % 16 == 4 * shift
        groups.append(dict(recon=(3.0 * gen(seed + g, Bk, n)).to(DEV), obs=torch.rand(Bk, n, generator=torch.Generator().manual_seed(
            seed + 10 + g)).to(DEV), out=out, logits=n != 7 and (g, n) != (1, 12), column=(g if n != 7 else 2)))
    return groups


def table_of(Bk, seed):
    """A random availability table; with three rows or more, one row holds nothing and one everything."""
    on = torch.rand(Bk, 3, generator=torch.Generator().manual_seed(seed)) < 0.5
    if Bk >= 3:
        on[1], on[Bk - 1] = False, True
    return on, availability_table(on, Bk, DEV)


def select_ref(groups, table, Bk, shift=0):
    """mmdyn_complete_select, one launch per group, on the same operands."""
    outs = []
    for g in groups:
        out = torch.full((g["recon"].numel() + 4,), float("nan"), device=DEV)[shift:shift + g["recon"].numel()].view_as(g["recon"])
        HIP.complete_select(g["obs"], g["recon"], table, g["column"], out, g["logits"])
        outs.append(out)
    return outs


# the issue's shapes: one pose row alone; three groups with every path of the quad loop (rows of 48 and the 7-float rows that
# straddle quads) under a table; more rows than a block holds quads, one group unobserved; destinations off the 16-byte boundary;
# the real frame (two 3 x 64 x 64 images and the pose)
@pytest.mark.parametrize("row_lens,Bk,shift,with_table,no_obs", [((7,), 1, 0, False, (0,)), ((48, 48, 7), 5, 0, True, ()),
                                                                  ((48, 48, 7), 37, 0, True, (1,)), ((12, 12), 3, 1, True, ()),
                                                                  ((12288, 12288, 7), 2, 0, True, ())])
def test_feed_is_complete_select_group_by_group(row_lens, Bk, shift, with_table, no_obs):
    """1. / 2. Each group's output has the bits of mmdyn_complete_select on the same operands; with NaN written over the side that
    must not be loaded (the recon row of an observed (row, group), the obs row of an unobserved one) the outputs are finite and
    the same bits."""
    groups = operands(Bk, row_lens, 900 + Bk, shift)
    for g in no_obs:
        groups[g]["obs"] = None
    on, table = table_of(Bk, 910 + Bk) if with_table else (torch.ones(Bk, 3, dtype=torch.bool), None)
    HIP.rollout_feed(groups, table, Bk)
    want = select_ref(groups, table, Bk, shift)
    for g, w in zip(groups, want):
        assert dirty.first_diff(g["out"], w) is None, (g["column"], dirty.first_diff(g["out"], w))
        assert bool(torch.isfinite(g["out"]).all())
    clean = [g["out"].clone() for g in groups]
    for g in groups:
        taken = on[:, g["column"]].to(DEV) if g["obs"] is not None else torch.zeros(Bk, dtype=torch.bool, device=DEV)
        g["recon"][taken] = float("nan")
        if g["obs"] is not None:
            g["obs"][~taken] = float("nan")
        g["out"].fill_(float("nan"))
    HIP.rollout_feed(groups, table, Bk)
    for g, c in zip(groups, clean):
        assert dirty.first_diff(g["out"], c) is None and bool(torch.isfinite(g["out"]).all()), g["column"]


def test_feed_on_dirty_destinations():
    """3. Zero-, NaN- and junk-filled destinations (tests/dirty.py): the same bits; the inputs and the table are not written."""
    Bk, row_lens = 5, (48, 48, 7)
    src = operands(Bk, row_lens, 930)
    _, table = table_of(Bk, 931)

    def feed(backend, r0, r1, r2, o0, o1, o2, d0, d1, d2, tab):
        backend.rollout_feed([dict(recon=r, obs=o, out=d, logits=g["logits"], column=g["column"])
                              for r, o, d, g in zip((r0, r1, r2), (o0, o1, o2), (d0, d1, d2), src)], tab, Bk)
    args = tuple(g["recon"] for g in src) + tuple(g["obs"] for g in src) + tuple(torch.empty(Bk, n) for n in row_lens) + (table,)
    runs = dirty.run_dirty(HIP, feed, args, outs=[6, 7, 8], device=DEV)
    dirty.assert_same_bits(runs, what="rollout_feed: ")


def test_feed_rejects_bad_arguments():
    """4. MMDYN_ERR_NULL / _SHAPE / _RANGE from the raw entry point, before any launch."""
    lib, t = HIP.lib, torch.zeros(64, device=DEV)
    p = t.data_ptr()

    def call(G=1, Bk=1, table=None, **over):
        a = _lib.FeedGroups()
        for g in range(4):
            a.recon[g], a.obs[g], a.out[g], a.row_len[g], a.logits[g], a.column[g] = p, None, p + 128, 4, 0, g
        for k, (g, v) in over.items():
            getattr(a, k)[g] = v
        return lib.mmdyn_rollout_feed(ctypes.addressof(a), G, table, Bk, None)
    assert lib.mmdyn_rollout_feed(None, 1, None, 1, None) == -2
    assert call(recon=(0, None)) == -2 and call(G=2, out=(1, None)) == -2
    assert call(G=0) == -1 and call(G=5) == -1 and call(Bk=0) == -1
    assert call(row_len=(0, 0)) == -1 and call(column=(0, 4)) == -1 and call(column=(0, -1)) == -1
    assert call(table=p + 1) == -1                                              # misaligned table
    assert call(out=(0, p)) == -1 and call(obs=(0, p + 128)) == -1 and call(out=(0, p + 8)) == -1      # out overlaps recon / obs
    assert call(Bk=32768, row_len=(0, 65536)) == -3                            # B * row_len = 2^31
    assert call(G=2, Bk=32768, row_len=(1, 65536), out=(0, p + (1 << 30))) == -3
    assert call(recon=(1, None)) == 0                                           # groups past G are not looked at
    torch.cuda.synchronize()


# ---- the engine ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    """What stands behind the decoders inherits their fp32 summation order: the bound this suite puts on such sums."""
    if a is None or b is None:
        return a is None and b is None
    return torch.allclose(a.double(), b.double(), rtol=RTOL_SUM, atol=0.0)


def test_one_step_consistency():
    """Sigmoid bound on the device as in tests/test_mixed_modal_gpu.py::test_complete: two fp32 evaluations, 4 * 2^-24 apart."""
    E.check_one_step_consistency(DEV, sigmoid_atol=4 * 2.0 ** -24)


def test_against_todays_calls():
    E.check_against_todays_calls(DEV, same)


def test_observation():
    E.check_observation(DEV, same)


def test_conditions():
    E.check_conditions(DEV)


def test_problem_layer():
    E.check_problem_layer(DEV)


def philox_draws(seed, first_block, n):
    """The T draws of one rollout call from the exact reference, rounded to fp32: step t sits at counter first_block + t * n."""
    return [torch.from_numpy(P.normal_ref(B * L, seed, first_block + t * n)[0].astype(np.float32)).reshape(B, L) for t in range(T)]


def test_captured_rollout_equals_eager_on_one_philox_stream():
    """9. use_graph=True against an eager engine with the same seed: three calls with new inputs, the KL weight changing at the
    third.  One graph is captured and its key carries T; replay c follows the inputs of call c.  Draw accounting: step t of eager
    call c draws at counter (c T + t) n with n = counters_of(B L); the capture's eager warm-up takes the first T blocks, so replay c
    is compared with eager call c + 1.  means / log_var of step 0 stand in front of every decoder: equal bit for bit; everything
    later stands behind the decoders: OUT_TOL (the engine-against-oracle bound) for the posteriors and states, RTOL_SUM for the
    tables.  The draws are tied to tests/philox_ref.py through ``means``: means[t + 1] is a function of the draw of step t, so a
    rollout with the reference's numbers INJECTED at the accounted counters must give the engine's means -- a device normal is
    within NORMAL_TOL (about 1e-6) of the reference, and a unit change of a draw moves the next posterior by about 0.05 (the
    median step-to-step change asserted below), so the injected run sits orders of magnitude inside OUT_TOL -- while the draws of
    the NEXT call's counters give means further away than 100 x the tolerance."""
    seed, n = 5, P.counters_of(B * L)
    assert NORMAL_TOL < 1e-4
    model = TMM.build(False, DEV)
    av = RC.start()[1]
    xs = [E.dev_list(RC.start(840 + c)[0], DEV) for c in range(3)]
    tgs = [E.dev_list(RC.frames(850 + c), DEV) for c in range(3)]
    weights = (0.3, 0.3, 2.0)
    call = lambda eng, c: E.keep(eng.rollout([xs[c][0], xs[c][1]], pose=xs[c][2], steps=T, available=av, sample=True, targets=tgs[c],
                                             kl_weight=weights[c], pose_multiplier=RC.POSE_MULTIPLIER))
    eager = MVAEInference(model, seed=seed, use_graph=False)
    e = [call(eager, c) for c in (0, 0, 1, 2)]
    graph = MVAEInference(model, seed=seed)
    assert graph.use_graph
    g = [call(graph, c) for c in range(3)]
    assert len(graph._graphs) == 1
    key = next(iter(graph._graphs))
    assert key[:3] == ("rollout", T, True)
    tol = TMM.OUT_TOL
    for c in range(3):
        a, b = g[c], e[c + 1]
        assert torch.equal(a["means"][0], b["means"][0]) and torch.equal(a["log_var"][0], b["log_var"][0]), c
        print("replay", c, "bit-equal to eager:", {k: bool(torch.equal(a[k], b[k])) for k in a})
        for k in ("means", "log_var", "visual", "tactile", "pose"):
            np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), **tol, err_msg=f"{k} {c}")
        for k in E.TERMS:
            assert same(a[k], b[k]), (c, k)
    assert not torch.equal(g[0]["means"][1:], g[1]["means"][1:]) and float((g[2]["rows"] - g[1]["rows"]).abs().min()) > 0
    # the same inputs again: fresh noise, so everything behind step 0's draw moves
    again = call(graph, 2)
    assert torch.equal(again["means"][0], g[2]["means"][0]) and not torch.equal(again["means"][1], g[2]["means"][1])
    assert len(graph._graphs) == 1
    inj = MVAEInference(model, use_graph=False)
    for who, res, first, inputs in (("eager", e, 0, (0, 0, 1, 2)), ("graph", g, 1, (0, 1, 2))):
        for c, r in enumerate(res):
            for block, near in ((c + first, True), (c + first + 1, False)):
                inj.noise = InjectedNoise(philox_draws(seed, block * T * n, n), [])
                x = xs[inputs[c]]
                m = inj.rollout([x[0], x[1]], pose=x[2], steps=T, available=av, sample=True)["means"]
                d = (m - r["means"]).abs()
                print(who, "call", c, "draws of block", block, "largest / median |means - injected|", float(d.max()), float(d[1:].median()))
                if near:
                    np.testing.assert_allclose(m.cpu().numpy(), r["means"].cpu().numpy(), **tol, err_msg=f"{who} {c}")
                else:
                    assert float(d[1:].median()) > 100 * tol["atol"], (who, c)
    graph.close(), eager.close(), inj.close()


def test_rollout_on_dirty_allocator_memory(monkeypatch):
    """10. Eager, mixed start, observed touch under a table, targets: every torch.empty of ops / layers / engine pre-filled with
    zeros, NaNs or junk (tests/dirty.py), and the real torch.empty: the same bits; the fp64 tables and the rows assembled from them
    come from atomics (rtol 1e-12)."""
    inputs, av = RC.start()
    inputs, eps = E.dev_list(inputs, DEV), RC.draws()
    obs, tgs, tab = E.dev_list(RC.frames(861), DEV), E.dev_list(RC.frames(862), DEV), RC.mixed_table(8)
    got = {}
    for fill in (None,) + dirty.FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else dirty.PoisonTorch(fill))
        eng = MVAEInference(TMM.build(False, DEV), use_graph=False)
        try:
            r = E.roll(eng, inputs, av, eps, observed=[None, obs[1], None], observed_available=tab, targets=tgs,
                       target_available=tab, **E.KW)
            torch.cuda.synchronize()
            got["real torch.empty" if fill is None else fill] = {k: v.detach().cpu().clone() for k, v in r.items()}
        finally:
            eng.close()
    dirty.assert_same_bits(got, approx=E.TERMS, what="rollout: ")
