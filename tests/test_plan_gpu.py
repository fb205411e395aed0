"""Candidate conditions on a real MI355X: mmdyn_concat_condition_tiled against mmdyn_concat_condition on the repeated features (bit
for bit), mmdyn_plan_select against its rules and its fp64 restatement, mmdyn_gather_best against mmdyn_complete_select on the rows
a torch index picks (bit for bit, with NaN on the rows it must not load); then ``MVAEInference.plan`` -- the checks of
tests/test_plan_emu.py on the HIP library, captured against eager on one Philox stream, a replay with new candidates, dirty
allocator memory -- and ``DynModeling.plan``.  The reference has no such operation: nothing here comes from a golden file."""
import ctypes

import numpy as np
import pytest
import torch

import dirty
import philox_ref as P
import plan_cases as PC
import test_plan_emu as E
from mmdyn_hip import _lib, engine, layers, ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from test_elbo_rows_gpu import RTOL_SUM          # (that file's constant, not a new one)
from test_noise_gpu import NORMAL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
L = PC.L
SIGMOID_ATOL = 4 * 2.0 ** -24                   # two fp32 evaluations of a sigmoid (tests/test_mixed_modal_gpu.py::test_complete)


def gen(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the tiled join ---------------------------------------------------------------------------------------------------------
def shifted(rows, width, shift):
    """A contiguous [rows][width] destination that starts ``shift`` floats past a 16-byte boundary."""
    out = torch.zeros(rows * width + 4, device=DEV)[shift:shift + rows * width].view(rows, width)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4 * shift
    return out


# (x_rows, N, K, ldx, cd, width, categorical, shift): one row; class indices with one out of range; a row stride past K; the
# element path; a destination off the 16-byte boundary
JOINS = [(1, 1, 512, 512, 3, 544, False, 0), (3, 5, 512, 512, 5, 544, True, 0), (37, 2, 512, 520, 3, 544, False, 0),
         (3, 4, 7, 7, 2, 32, False, 0), (3, 2, 512, 512, 3, 544, False, 1)]


@pytest.mark.parametrize("x_rows,N,K,ldx,cd,width,categorical,shift", JOINS)
def test_tiled_join_is_the_join_of_the_repeated_rows(x_rows, N, K, ldx, cd, width, categorical, shift):
    rows = x_rows * N
    x = gen(100 + x_rows, x_rows, ldx).to(DEV)[:, :K]
    if categorical:
        cond = (torch.arange(rows) % cd).to(torch.int64)
        cond[rows - 2] = cd                                               # one index out of range
        cond = cond.to(DEV)
    else:
        cond = gen(200 + N, rows, cd).to(DEV)
    bad = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2)]
    got, want = shifted(rows, width, shift).fill_(float("nan")), shifted(rows, width, shift).fill_(float("nan"))
    HIP.concat_condition_tiled(x, cond, got, K, cd, x_rows, bad[0] if categorical else None)
    HIP.concat_condition(x.repeat(N, 1), cond, want, K, cd, bad[1] if categorical else None)
    assert dirty.first_diff(got, want) is None, dirty.first_diff(got, want)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[:, :K], x.repeat(N, 1)) and float(got[:, K + cd:].abs().sum()) == 0.0
    if categorical:
        assert int(bad[0].item()) == 1 == int(bad[1].item())
        assert float(got[rows - 2, K:K + cd].abs().sum()) == 0.0 and float(got[0, K:K + cd].sum()) == 1.0
    # x_rows == rows is the plain join
    plain = shifted(rows, width, shift)
    HIP.concat_condition_tiled(x.repeat(N, 1), cond, plain, K, cd, rows, bad[0] if categorical else None)
    assert dirty.first_diff(plain, want) is None


def test_tiled_join_on_dirty_destinations_and_bad_arguments():
    x_rows, N, K, cd, width = 3, 4, 40, 3, 64
    args = (gen(1, x_rows, K), gen(2, x_rows * N, cd), torch.empty(x_rows * N, width), K, cd, x_rows)
    dirty.assert_same_bits(dirty.run_dirty(HIP, "concat_condition_tiled", args, outs=[2], device=DEV), what="concat_condition_tiled: ")
    lib, t = HIP.lib, torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    call = lambda rows, xr: lib.mmdyn_concat_condition_tiled(p, p, None, p + 8192, None, rows, xr, 8, 8, 2, 32, None)
    assert call(7, 3) == -1 and call(6, 0) == -1 and call(6, 4) == -1          # rows is not a multiple of x_rows
    assert lib.mmdyn_concat_condition_tiled(p, p, p, p + 8192, None, 6, 3, 8, 8, 2, 32, None) == -2      # two condition sources
    assert lib.mmdyn_concat_condition_tiled(None, p, None, p + 8192, None, 6, 3, 8, 8, 2, 32, None) == -2
    assert lib.mmdyn_concat_condition_tiled(p, p, None, p + 8192, None, 1 << 26, 1, 8, 8, 2, 32, None) == -3
    assert call(6, 3) == 0
    torch.cuda.synchronize()


# ---- plan_select ------------------------------------------------------------------------------------------------------------
def test_select_rules():
    E.check_select_rules(HIP, DEV)


def test_select_cost_is_not_contracted():
    E.check_select_no_contraction(HIP, DEV)


@pytest.mark.parametrize("B,N", [(1, 1), (5, 9), (300, 2)])
def test_select_against_the_restatement(B, N):
    E.check_select_restatement(HIP, DEV, B, N)


def test_select_on_dirty_destinations_and_bad_arguments():
    N, B = 3, 5
    bce, mse, kl = PC.random_tables(B, N, 7)
    tab = torch.ones(B, 4, dtype=torch.uint8)
    tab[1, 0] = tab[3, 2] = 0
    args = (bce, mse, kl, tab, gen(3, N * B, 2), torch.empty(N, B), torch.empty(B, dtype=torch.int32), torch.empty(B), torch.empty(B, 2),
            N, B, 1000.0, 0.3)
    runs = dirty.run_dirty(HIP, "plan_select", args, outs=[5, 6, 7, 8], state=[0, 1], device=DEV)
    dirty.assert_same_bits(runs, what="plan_select: ")
    lib, t = HIP.lib, torch.zeros(256, device=DEV)
    p = t.data_ptr()
    f = lambda kl=p, tav=None, cand=p, idx=None, cost=p, best=p, bc=p, cond=p, bidx=None, N=1, B=1, cd=1: lib.mmdyn_plan_select(
        None, None, kl, tav, cand, idx, cd, cost, best, bc, cond, bidx, N, B, 1.0, 1.0, None, None)
    assert f(kl=None) == -2 and f(cost=None) == -2 and f(best=None) == -2 and f(bc=None) == -2
    assert f(cand=None, cond=None) == -2 and f(idx=p, bidx=p) == -2 and f(cond=None) == -2 and f(cand=None, cond=None, idx=p) == -2
    assert f(N=0) == -1 and f(B=0) == -1 and f(cd=0) == -1 and f(tav=p + 1) == -1
    assert f(N=65536, B=32768) == -3
    torch.cuda.synchronize()


# ---- gather_best ------------------------------------------------------------------------------------------------------------
def gather_operands(row_lens, B, N, seed, shift=0):
    groups = []
    for g, n in enumerate(row_lens):
        groups.append(dict(src=(3.0 * gen(seed + g, N * B, n)).to(DEV), out=shifted(B, n, shift), logits=n != 7 and (g, n) != (1, 12)))
    best = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    if B >= 3:
        best[1] = -1                                                     # a row without a winner
    return groups, best.to(DEV)


@pytest.mark.parametrize("row_lens,B,N,shift", [((48, 48, 7), 5, 3, 0), ((12288, 12288, 7), 2, 2, 0), ((12, 12), 3, 3, 1)])
def test_gather_is_complete_select_on_the_picked_rows(row_lens, B, N, shift):
    """Each group against mmdyn_complete_select(x = null) on the rows a torch index picks: the same bits in every taken row; a row
    with best = -1 is all NaN; with NaN written over every source row that is not taken the output is finite and unchanged."""
    groups, best = gather_operands(row_lens, B, N, 950 + B, shift)
    taken = best >= 0
    rows = torch.where(taken, best.long(), torch.zeros_like(best).long()) * B + torch.arange(B, device=DEV)
    HIP.gather_best(groups, best, N, B)
    for g in groups:
        want = shifted(B, g["src"].shape[1], shift)
        HIP.complete_select(None, g["src"][rows], None, 0, want, g["logits"])
        assert dirty.first_diff(g["out"][taken], want[taken]) is None, dirty.first_diff(g["out"][taken], want[taken])
        assert bool(torch.isfinite(g["out"][taken]).all()) and bool(torch.isnan(g["out"][~taken]).all())
    clean = [g["out"].clone() for g in groups]
    for g in groups:
        keep = torch.zeros(N * B, dtype=torch.bool, device=DEV)
        keep[rows[taken]] = True
        g["src"][~keep] = float("nan")
        g["out"].fill_(0.0)
    HIP.gather_best(groups, best, N, B)
    for g, c in zip(groups, clean):
        assert dirty.first_diff(g["out"], c) is None
    # hand-made indices outside [-1, N): NaN rows, nothing read out of bounds
    wild = best.clone()
    wild[0] = N
    wild[B - 1] = -(2 ** 31)
    HIP.gather_best(groups, wild, N, B)
    for g in groups:
        assert bool(torch.isnan(g["out"][0]).all()) and bool(torch.isnan(g["out"][B - 1]).all())


def test_gather_on_dirty_destinations_and_bad_arguments():
    B, N, row_lens = 5, 3, (48, 48, 7)
    src, best = gather_operands(row_lens, B, N, 960)
    best[1] = 0

    def gather(backend, s0, s1, s2, d0, d1, d2, bst):
        backend.gather_best([dict(src=s, out=d, logits=g["logits"]) for s, d, g in zip((s0, s1, s2), (d0, d1, d2), src)], bst, N, B)
    args = tuple(g["src"] for g in src) + tuple(torch.empty(B, n) for n in row_lens) + (best,)
    dirty.assert_same_bits(dirty.run_dirty(HIP, gather, args, outs=[3, 4, 5], device=DEV), what="gather_best: ")
    lib, t = HIP.lib, torch.zeros(1024, device=DEV)
    p, ip = t.data_ptr(), torch.zeros(8, dtype=torch.int32, device=DEV).data_ptr()

    def call(G=1, N=2, Bk=1, best=ip, **over):
        a = _lib.GatherGroups()
        for g in range(4):
            a.src[g], a.out[g], a.row_len[g], a.logits[g] = p, p + 2048, 4, 0
        for k, (g, v) in over.items():
            getattr(a, k)[g] = v
        return lib.mmdyn_gather_best(ctypes.addressof(a), G, best, N, Bk, None)
    assert lib.mmdyn_gather_best(None, 1, ip, 1, 1, None) == -2 and call(best=None) == -2
    assert call(src=(0, None)) == -2 and call(G=2, out=(1, None)) == -2
    assert call(G=0) == -1 and call(G=5) == -1 and call(Bk=0) == -1 and call(N=0) == -1 and call(row_len=(0, 0)) == -1
    assert call(out=(0, p)) == -1 and call(out=(0, p + 16)) == -1 and call(out=(0, p + 28)) == -1      # out inside the N * B source rows
    assert call(out=(0, ip)) == -1                                              # out over the indices
    # two groups: an out may touch neither the other group's source rows nor its out
    assert call(G=2, src=(1, p + 512), out=(1, p + 3072)) == 0
    assert call(G=2, src=(1, p + 512), out=(1, p + 8)) == -1 and call(G=2, src=(1, p + 3072 - 16), out=(1, p + 3072)) == -1
    assert call(G=2, src=(1, p + 512)) == -1 and call(G=2, src=(1, p + 2048 - 16), out=(1, p + 3072)) == -1
    assert call(N=32768, row_len=(0, 65536)) == -3
    assert call(src=(1, None)) == 0                                             # groups past G are not looked at
    torch.cuda.synchronize()


# ---- the engine ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    """What stands behind the decoders inherits their fp32 summation order: the bound this suite puts on such sums."""
    return torch.allclose(a.double(), b.double(), rtol=RTOL_SUM, atol=0.0)


@pytest.mark.parametrize("name,sample", [("classes", False), ("shared", True), ("per_row", False), ("one", True)])
def test_plan_against_the_oracle(name, sample):
    E.check_against_oracle(DEV, name, sample, sigmoid_atol=SIGMOID_ATOL)


def test_mixed_request_and_absent_goal_terms():
    E.check_against_oracle(DEV, "shared", True, mixed=True, sigmoid_atol=SIGMOID_ATOL)


@pytest.mark.parametrize("name", ["classes", "per_row", "one"])
def test_plan_against_separate_requests(name):
    E.check_against_separate_requests(DEV, name, sigmoid_atol=SIGMOID_ATOL)


def test_permuted_candidates():
    E.check_permutation(DEV)


def test_problem_layer():
    E.check_problem_layer(DEV)


def test_captured_plan_equals_eager_on_one_philox_stream():
    """use_graph=True against an eager engine with the same seed: three calls with new inputs AND new candidate values of the same
    shape, the KL weight changing at the third.  One graph is captured, its key carries N and the kind of the candidates, not their
    values; replay c follows the inputs and the candidates of call c.  Draw accounting: sample=True takes ONE [B, L] block per
    call, n = counters_of(B L) counters; the capture's eager warm-up takes the first block, so replay c is compared with eager call
    c + 1.  means / log_var stand in front of every decoder: equal bit for bit; the tables stand behind them: RTOL_SUM; ``best``
    equal.  The draw is tied to tests/philox_ref.py through the pose outputs, which move by about 0.1 under another draw: a
    request with the reference's numbers INJECTED at the accounted counter gives the engine's pose rows within OUT_TOL, the
    numbers of the NEXT block give rows further away than 100 x the tolerance."""
    name, seed = "shared", 5
    B, N, categorical, _ = PC.CASES[name]
    n = P.counters_of(B * L)
    assert NORMAL_TOL < 1e-4
    model = PC.build(categorical, DEV)
    from mmdyn_hip.utils.seeded_init import seeded_batch
    xs = [E.dev_list(seeded_batch(B, 970 + c, with_pose=True)[0], DEV) for c in range(3)]
    goals = [E.dev_list(seeded_batch(B, 980 + c, with_pose=True)[1], DEV) for c in range(3)]
    cands = [torch.rand(N, 3, generator=torch.Generator().manual_seed(990 + c)).to(DEV) for c in range(3)]
    weights = (0.3, 0.3, 2.0)
    call = lambda eng, c: E.keep(eng.plan([xs[c][0], xs[c][1]], pose=xs[c][2], goal=goals[c], candidates=cands[c], sample=True,
                                          kl_weight=weights[c], pose_multiplier=PC.POSE_MULTIPLIER))
    eager = MVAEInference(model, seed=seed, use_graph=False)
    e = [call(eager, c) for c in (0, 0, 1, 2)]
    graph = MVAEInference(model, seed=seed)
    assert graph.use_graph
    g = [call(graph, c) for c in range(3)]
    assert len(graph._graphs) == 1
    key = next(iter(graph._graphs))
    assert key[0] == "plan" and ("candidates", N, False) in key and "real" in key
    for c in range(3):
        a, b = g[c], e[c + 1]
        assert torch.equal(a["means"], b["means"]) and torch.equal(a["log_var"], b["log_var"]), c
        print("replay", c, "bit-equal to eager:", {k: bool(torch.equal(a[k], b[k])) for k in ("cost", "best", "kl", "bce_visual")})
        for k in E.TERMS + ("cost", "best_cost"):
            assert same(a[k], b[k]), (c, k)
        low = b["cost"].double().min(0).values.abs().cpu()
        assert bool((PC.gap(b["cost"].double().cpu()) >= E.GAP * low).all())    # (the choice is pinned: the gap condition)
        assert torch.equal(a["best"], b["best"]) and torch.equal(a["best_condition"], b["best_condition"]), c
        win = a["best"].long()
        assert torch.equal(a["best_condition"], cands[c][win])                  # the replay saw the new candidates
        for m in range(3):
            np.testing.assert_allclose(a["prediction"][m].cpu().numpy(), b["prediction"][m].cpu().numpy(), **E.OUT_TOL)
    assert not torch.equal(g[0]["cost"], g[1]["cost"]) and float((g[2]["cost"] - g[1]["cost"]).abs().min()) > 0
    # new candidate values alone, same inputs: the same posterior-independent inputs, another table
    again = E.keep(graph.plan([xs[2][0], xs[2][1]], pose=xs[2][2], goal=goals[2], candidates=cands[0], sample=True, kl_weight=2.0,
                              pose_multiplier=PC.POSE_MULTIPLIER))
    assert len(graph._graphs) == 1 and torch.equal(again["best_condition"], cands[0][again["best"].long()])
    assert not torch.equal(again["means"], g[2]["means"])
    inj = MVAEInference(model, use_graph=False)
    draw = lambda block: torch.from_numpy(P.normal_ref(B * L, seed, block * n)[0].astype(np.float32)).reshape(B, L)
    tol = E.OUT_TOL
    for who, res, first, inputs in (("eager", e, 0, (0, 0, 1, 2)), ("graph", g, 1, (0, 1, 2))):
        for c, r in enumerate(res):
            for block, near in ((c + first, True), (c + first + 1, False)):
                inj.noise = InjectedNoise([draw(block)], [])
                i = inputs[c]
                pr = inj.plan([xs[i][0], xs[i][1]], pose=xs[i][2], goal=goals[i], candidates=cands[i], sample=True)["recon_x"][2]
                d = (pr - r["recon_x"][2]).abs()
                print(who, "call", c, "draws of block", block, "largest / median |pose - injected|", float(d.max()), float(d.median()))
                if near:
                    np.testing.assert_allclose(pr.cpu().numpy(), r["recon_x"][2].cpu().numpy(), **tol, err_msg=f"{who} {c}")
                else:
                    assert float(d.median()) > 100 * tol["atol"], (who, c)
    graph.close(), eager.close(), inj.close()


def test_plan_on_dirty_allocator_memory(monkeypatch):
    """Eager, the mixed request with absent goal terms: every torch.empty of ops / layers / engine pre-filled with zeros, NaNs or
    junk (tests/dirty.py), and the real torch.empty: the same bits; the fp64 tables and what is assembled from them come from
    atomics (rtol 1e-12)."""
    name = "shared"
    eps = PC.request(name)[3]
    got = {}
    for fill in (None,) + dirty.FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else dirty.PoisonTorch(fill))
        eng = MVAEInference(PC.build(False, DEV), use_graph=False)
        try:
            r = E.ask(eng, name, DEV, eps, **E.mixed_tables())
            torch.cuda.synchronize()
            flat = {}
            for k, v in r.items():
                for i, t in enumerate(v if isinstance(v, list) else [v]):
                    flat[f"{k}{i}" if isinstance(v, list) else k] = t.detach().cpu().clone()
            got["real torch.empty" if fill is None else fill] = flat
        finally:
            eng.close()
    dirty.assert_same_bits(got, approx=E.TERMS + ("cost", "best_cost"), what="plan: ")
