"""Importance-weighted K-sample bound on a real MI355X: mmdyn_iw_latent and mmdyn_iw_assemble_rows against the fp64 restatements of
tests/iw_cases.py and against identities that hold exactly, then ``MVAEInference.score(samples=K)`` -- eager against the restatement
on the oracle's eval-mode forward and against today's ``score()`` called once per draw, captured against eager on one Philox stream,
and on dirty allocator memory.  The reference has no such estimator: nothing here comes from a golden file."""
import math

import numpy as np
import pytest
import torch

import dirty
import iw_cases as IW
import philox_ref as P
import test_iw_bound_emu as E
import test_mixed_modal_emu as TMM
from mmdyn_hip import engine, layers, ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models.functional import availability_table
from test_elbo_rows_gpu import RTOL_SAME, RTOL_SUM          # (that file's constants, not new ones)
from test_noise_gpu import NORMAL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B


def gen(seed, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def heads(B, L, ld, seed):
    """(mu, lv) on the device as rows of stride ld: separate tensors for ld == L, the two halves of one [B][2L] tensor otherwise."""
    if ld == L:
        return gen(seed, B, L).to(DEV), (0.5 * gen(seed + 1, B, L) - 0.5).to(DEV)
    assert ld == 2 * L
    h = torch.cat((gen(seed, B, L), 0.5 * gen(seed + 1, B, L) - 0.5), 1).to(DEV)
    return h[:, :L], h[:, L:]


# the issue's four shapes (one row; odd K and B on contiguous heads; L no multiple of the 256-float wave trip on fused heads; many
# draws of few rows) + the two shapes at which the launch takes its element-wise path: L % 4 != 0, and an eps pointer off 16 bytes
@pytest.mark.parametrize("K,B,L,ld,shift", [(1, 1, 32, 32, 0), (3, 5, 256, 256, 0), (5, 37, 96, 192, 0), (64, 2, 256, 512, 0),
                                            (2, 3, 30, 30, 0), (3, 5, 64, 128, 1)])
def test_iw_latent(K, B, L, ld, shift):
    """z bit-equal to mmdyn_reparam_fwd's on the same mu, lv, eps_k for each k; |ratio - ref| <= 1e-12 * sum_l |terms| with the
    reference summed in fp64 from the kernel's own z (the only difference is the fp64 summation order: RTOL_SAME on the sum of
    magnitudes, because the sum itself may cancel); two runs give the same bits; ratio and z pre-filled with NaN change nothing."""
    mu, lv = heads(B, L, ld, 600 + K)
    eps = torch.zeros(K * B * L + 4, device=DEV)[shift:shift + K * B * L].view(K, B, L)
    eps.copy_(gen(610 + B, K, B, L))
    z, ratio = torch.zeros(K, B, L, device=DEV), torch.zeros(K, B, dtype=torch.float64, device=DEV)
    assert eps.is_contiguous() and eps.data_ptr() % 16 == 4 * shift
    call = lambda z_, r_: HIP.iw_latent(mu, lv, eps, z_, r_, K, B, L)
    call(z, ratio)
    for k in range(K):
        zk = torch.empty(B, L, device=DEV)
        HIP.reparam_fwd(mu, lv, eps[k], zk, None, B, L, ld)
        assert torch.equal(z[k], zk), (k, int((z[k] != zk).sum()))
    want, mag = IW.iw_ratio_ref(z.cpu(), eps.cpu(), lv.cpu())
    err = (ratio.cpu() - want).abs()
    print("iw_latent", (K, B, L, ld, shift), "largest |ratio - ref| / sum|terms|", float((err / mag).max()))
    assert bool((err <= RTOL_SAME * mag).all())
    z2, r2 = torch.full_like(z, float("nan")), torch.full_like(ratio, float("nan"))
    call(z2, r2)
    assert dirty.first_diff(z2, z) is None and dirty.first_diff(r2, ratio) is None


def test_iw_latent_rejects_bad_arguments():
    lib, t = HIP.lib, torch.zeros(8, device=DEV)
    p = t.data_ptr()
    assert lib.mmdyn_iw_latent(None, p, 4, p, p, p, 1, 1, 4, None) == -2
    assert lib.mmdyn_iw_latent(p, p, 4, p, p, None, 1, 1, 4, None) == -2
    assert lib.mmdyn_iw_latent(p, p, 3, p, p, p, 1, 1, 4, None) == -1                       # row stride below L
    assert lib.mmdyn_iw_latent(p, p, 4, p, p, p, 0, 1, 4, None) == -1
    assert lib.mmdyn_iw_latent(p, p, 256, p, p, p, 65536, 128, 256, None) == -3             # K * B * L = 2^31: before any launch
    assert lib.mmdyn_iw_assemble_rows(None, None, None, None, p, None, None, 0, 1, 1, 1.0, 1.0, None, None) == -2
    assert lib.mmdyn_iw_assemble_rows(None, None, p, None, None, None, None, 0, 1, 1, 1.0, 1.0, None, None) == -2
    assert lib.mmdyn_iw_assemble_rows(p, None, p, None, p, None, None, 3, 1, 1, 1.0, 1.0, None, None) == -1
    assert lib.mmdyn_iw_assemble_rows(None, None, p, p + 1, p, None, None, 0, 1, 1, 1.0, 1.0, None, None) == -1   # misaligned table
    assert lib.mmdyn_iw_assemble_rows(None, None, p, None, p, None, None, 0, 65536, 32768, 1.0, 1.0, None, None) == -3


def test_mean_ratio_is_the_analytic_kl():
    """E_q[ratio] = KL(q || p): at K = 4096, B = 2, L = 32 with Philox draws of a fixed seed from mmdyn_random_normal,
    |mean_k ratio_k - kl_rows| <= 6 * std_k(ratio) / sqrt(K), the standard deviation taken from the sample.  Deterministic (fixed
    seed).  On the CPU, with tests/philox_ref.py draws and the restatement of tests/iw_cases.py, the two rows sit 0.41 and 0.48
    standard errors from their KL (17.76 / 12.27 against means of 17.73 / 12.24, std 4.43 / 4.23): a margin of a factor 12."""
    K, B, L, seed = 4096, 2, 32, 2024
    g = torch.Generator().manual_seed(901)
    mu, lv = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g) * 0.5 - 0.5
    mud, lvd = mu.to(DEV), lv.to(DEV)
    eps = torch.empty(K, B, L, device=DEV)
    HIP.random_normal(eps, seed, 0)
    z, ratio = torch.empty(K, B, L, device=DEV), torch.empty(K, B, dtype=torch.float64, device=DEV)
    HIP.iw_latent(mud, lvd, eps, z, ratio, K, B, L)
    kl = torch.empty(1, B, dtype=torch.float64, device=DEV)
    HIP.kl_rows(mud, lvd, kl, 1, B, L)
    ratio, kl = ratio.cpu(), kl.cpu()[0]
    dev, se = (ratio.mean(0) - kl).abs(), ratio.std(0) / math.sqrt(K)
    print("mean ratio", ratio.mean(0).tolist(), "kl", kl.tolist(), "standard errors off", (dev / se).tolist())
    assert bool((dev <= 6.0 * se).all())
    # the CPU side of the same statement, from the exact Philox reference
    eps_ref = torch.from_numpy(P.normal_ref(K * B * L, seed, 0)[0].astype(np.float32)).reshape(K, B, L)
    _, ratio_ref = IW.iw_latent_ref(mu, lv, eps_ref)
    kl_ref = -0.5 * (1 + lv.double() - mu.double() ** 2 - lv.double().exp()).sum(1)
    assert bool(((ratio_ref.mean(0) - kl_ref).abs() <= 6.0 * ratio_ref.std(0) / math.sqrt(K)).all())


def tables(K, B, seed):
    """Row tables with rec = bce_visual + bce_tactile + 1000 * mse of about 8000 +- 50 (exp(-8000) underflows: a sum without the
    maximum taken out gives +inf) and ratios of about 20 +- 5."""
    r = lambda s: torch.rand(K, B, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + s))
    bce = torch.stack((3500.0 + 40.0 * (r(0) - 0.5), 3490.0 + 40.0 * (r(1) - 0.5)))
    return bce, 1.0 + 0.02 * (r(2) - 0.5), 20.0 + 10.0 * (r(3) - 0.5)


def f32_weight(arg, dev):
    """The KL weight as the kernels form it: the fp32 product of the argument and the device word."""
    return float(torch.tensor(arg, dtype=torch.float32) * torch.tensor(dev, dtype=torch.float32))


def assemble(bce, mse, ratio, K, B, pm, klw_arg=1.0, klw_dev=None, tavail=None, with_ess=True, with_log_w=True):
    d = lambda t: None if t is None else t.to(DEV)
    bd, md, rd = d(bce), d(mse), d(ratio)
    out = torch.full((B,), float("nan"), device=DEV)
    ess = torch.full((B,), float("nan"), device=DEV) if with_ess else None
    lw = torch.full((K, B), float("nan"), dtype=torch.float64, device=DEV) if with_log_w else None
    HIP.iw_assemble_rows(bd, md, rd, tavail, out, ess, lw, K, B, pm, klw_arg, klw_dev)
    c = lambda t: None if t is None else t.cpu()
    return c(out), c(ess), c(lw), c(bd), c(md)


def close_to_ref(out, ess, lw, ref, K):
    """log_w: relative 1e-12; out: within 1e-12 * max_k |log_w_k| of the reference before the fp32 cast, i.e. between the fp32
    roundings of the reference moved by that much; ess: d ln(ess) = 2 sum_k (p_k - q_k) d log_w_k for two sets of normalised
    weights p, q, so at most 4 max_k |d log_w_k| = 4e-12 * max_k |log_w_k| relative, then the fp32 cast."""
    ref_out, ref_ess, ref_lw = ref[:3]
    assert torch.allclose(lw, ref_lw, rtol=1e-12, atol=0.0)
    tol = 1e-12 * torch.where(torch.isfinite(ref_lw), ref_lw.abs(), torch.zeros_like(ref_lw)).max(0).values
    print("K", K, "largest |out - float32(ref)|", float((out.double() - ref_out.float().double()).abs().max()))
    assert bool(((out >= (ref_out - tol).float()) & (out <= (ref_out + tol).float())).all())
    assert bool(((ess >= (ref_ess * (1 - 4 * tol)).float()) & (ess <= (ref_ess * (1 + 4 * tol)).float())).all())


@pytest.mark.parametrize("K,B", [(1, 1), (2, 5), (5, 37), (64, 3)])
def test_iw_assemble_rows(K, B):
    pm, klw_arg, klw_dev = 1000.0, 0.5, 0.04
    bce, mse, ratio = tables(K, B, 800 + K)
    dev_w = torch.tensor([klw_dev], device=DEV)
    out, ess, lw, bd, md = assemble(bce, mse, ratio, K, B, pm, klw_arg, dev_w)
    assert torch.equal(bd, bce) and torch.equal(md, mse)                                   # no table, nothing absent: read only
    ref = IW.iw_assemble_ref(bce, mse, ratio, None, pm, f32_weight(klw_arg, klw_dev))
    assert float(lw.max()) < -7900 and bool(torch.isfinite(out).all())                      # (exp(log_w) itself is 0 in fp64)
    close_to_ref(out, ess, lw, ref, K)
    # Jensen on the kernel's own outputs (fp32 rounding is monotone): min_k(-log_w_k) - log K <= out <= mean_k(-log_w_k)
    assert bool((out >= ((-lw).min(0).values - math.log(K)).float()).all()) and bool((out <= (-lw).mean(0).float()).all())
    assert float(ess.min()) >= 1.0 and float(ess.max()) <= K
    if K == 1:
        rec = bce[0] + bce[1] + pm * mse
        assert torch.equal(out, (rec + f32_weight(klw_arg, klw_dev) * ratio)[0].float()) and torch.equal(ess, torch.ones(B))
    # the KL weight is read from device memory: the same call, another value in the word, another result
    dev_w.fill_(1.5)
    out2, ess2, lw2, _, _ = assemble(bce, mse, ratio, K, B, pm, klw_arg, dev_w)
    close_to_ref(out2, ess2, lw2, IW.iw_assemble_ref(bce, mse, ratio, None, pm, f32_weight(klw_arg, 1.5)), K)
    assert float((out2 - out).abs().min()) > 0
    # optional outputs and optional terms
    out3, _, _, _, _ = assemble(bce, mse, ratio, K, B, pm, klw_arg, dev_w, with_ess=False, with_log_w=False)
    assert torch.equal(out3, out2)
    o_b, e_b, l_b, _, _ = assemble(bce[:1].contiguous(), None, ratio, K, B, pm, 1.0)
    close_to_ref(o_b, e_b, l_b, IW.iw_assemble_ref(bce[:1], None, ratio, None, pm, 1.0), K)
    o_r, e_r, l_r, _, _ = assemble(None, None, ratio, K, B, pm, 1.0)
    close_to_ref(o_r, e_r, l_r, IW.iw_assemble_ref(None, None, ratio, None, pm, 1.0), K)


def test_iw_assemble_rows_target_availability():
    """A (row, term) whose target is absent is left out of every log_w_k and its K table entries become 0; present entries keep
    their bits; a row with every term absent is -(lse_k(-kl_weight ratio_k) - log K), at kl_weight = 1 minus the log-mean-exp of
    -ratio."""
    K, B, pm = 5, 37, 1000.0
    bce, mse, ratio = tables(K, B, 840)
    on = torch.rand(B, 3, generator=torch.Generator().manual_seed(841)) < 0.6
    on[0], on[1], on[B - 1] = False, True, False
    table = availability_table(on, B, DEV)
    for klw in (0.25, 1.0):
        out, ess, lw, bd, md = assemble(bce, mse, ratio, K, B, pm, klw, None, tavail=table)
        ref = IW.iw_assemble_ref(bce, mse, ratio, on, pm, f32_weight(klw, 1.0))
        close_to_ref(out, ess, lw, ref, K)
        assert torch.equal(bd, ref[3]) and torch.equal(md, ref[4])
        for m, t in enumerate((bd[0], bd[1], md)):
            assert float(t[:, ~on[:, m]].abs().max()) == 0.0 and bool((t[:, on[:, m]] > 0).all())
    lme = torch.logsumexp(-ratio[:, 0], 0) - math.log(K)
    assert abs(float(out[0]) - float(-lme)) <= 1e-6 * abs(float(lme))


def test_iw_assemble_rows_zero_weights_and_nan():
    """A log_w of -inf is a zero weight; a row whose weights are all zero: out = +inf, ess = NaN; NaN propagates; the other rows
    do not notice."""
    K, B, pm = 4, 6, 1000.0
    bce, mse, ratio = tables(K, B, 860)
    clean = assemble(bce, mse, ratio, K, B, pm, 1.0)
    bce = bce.clone()
    bce[0, 1, 0] = float("inf")                  # row 0: one draw of infinite loss
    bce[1, :, 2] = float("inf")                  # row 2: every draw
    bce[0, 3, 4] = float("nan")                  # row 4
    out, ess, lw, _, _ = assemble(bce, mse, ratio, K, B, pm, 1.0)
    ref = IW.iw_assemble_ref(bce, mse, ratio, None, pm, 1.0)
    assert float(lw[1, 0]) == float("-inf") and math.isfinite(float(out[0])) and 1.0 <= float(ess[0]) <= K - 1
    keep = torch.tensor([0, 1, 3, 5])
    close_to_ref(out[keep], ess[keep], lw[:, keep], (ref[0][keep], ref[1][keep], ref[2][:, keep]), K)
    assert float(out[2]) == float("inf") and math.isnan(float(ess[2]))
    assert math.isnan(float(out[4])) and math.isnan(float(ess[4]))
    for b in (1, 3, 5):
        assert float(out[b]) == float(clean[0][b]) and float(ess[b]) == float(clean[1][b])


def test_kernels_on_dirty_destinations():
    """Both launches on zero-, NaN- and junk-filled outputs (tests/dirty.py): the same bits.  The row tables of the assembly are
    state: only the entries of absent terms change."""
    K, B, L = 3, 5, 64
    mu, lv = gen(880, B, L), 0.5 * gen(881, B, L) - 0.5
    runs = dirty.run_dirty(HIP, "iw_latent", (mu, lv, gen(882, K, B, L), torch.empty(K, B, L), torch.empty(K, B, dtype=torch.float64),
                                              K, B, L), outs=[3, 4], device=DEV)
    dirty.assert_same_bits(runs, what="iw_latent: ")
    bce, mse, ratio = tables(K, B, 883)
    on = torch.rand(B, 3, generator=torch.Generator().manual_seed(884)) < 0.6
    args = (bce, mse, ratio, availability_table(on, B, "cpu"), torch.empty(B), torch.empty(B), torch.empty(K, B, dtype=torch.float64),
            K, B, 1000.0, 0.5, torch.tensor([0.04]))
    runs = dirty.run_dirty(HIP, "iw_assemble_rows", args, outs=[4, 5, 6], state=[0, 1], device=DEV)
    dirty.assert_same_bits(runs, what="iw_assemble_rows: ")


# ---- the engine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("joint", "fp32"), ("joint", "fp32x3"), ("visual_targets", "fp32x3"), ("mixed", "fp32x3"),
                                            ("categorical", "fp32x3"), ("mask1", "fp32x3")])
def test_score_samples_against_the_restatement(name, precision):
    E.check_engine_case(DEV, name, precision)


def test_problem_iw_score():
    E.check_problem_iw_score(DEV)


def philox_ratio(means, log_var, K, seed, block):
    """(ratio, bound) of the draw at Philox counter ``block`` from the exact reference.  A device normal is within NORMAL_TOL of
    the reference (tests/test_noise_gpu.py) and the reference is rounded to fp32 here: d eps <= NORMAL_TOL + 2^-24 |eps|; the device's
    expf is within an ulp of torch's: d z <= exp(lv / 2) d eps + 2^-22 |z|; to first order d ratio <= sum_l |z| d z + |eps| d eps."""
    B, L = means.shape
    eps = torch.from_numpy(P.normal_ref(K * B * L, seed, block)[0].astype(np.float32)).reshape(K, B, L)
    z, ratio = IW.iw_latent_ref(means, log_var, eps)
    d_eps = NORMAL_TOL + 2.0 ** -24 * eps.abs().double()
    d_z = torch.exp(0.5 * log_var.double()).unsqueeze(0) * d_eps + 2.0 ** -22 * z.abs().double()
    return ratio, (z.abs().double() * d_z + eps.abs().double() * d_eps).sum(2)


def test_captured_score_equals_eager_on_one_philox_stream():
    """use_graph=True against an eager engine with the same seed over three calls, the KL weight changing at the third: one
    capture serves them, consecutive replays differ (fresh noise), and the draws are the Philox blocks the accounting says: an
    eager call c draws at counter c * ceil(K B L / 4); the capture's eager warm-up pass takes block 0, so replay c draws block c + 1
    and is compared with eager call c + 1.  What no atomic and no GEMM touches after the encoders (means, log_var, kl, ratio) is equal
    bit for bit; the row tables, log_w, rows and the sample size stand behind the decoders, whose repeatability from run to run this
    suite does not claim: they inherit the decoders' fp32 summation order, the bound the suite puts on such sums (RTOL_SUM)."""
    B, K, seed = 3, 2, 5
    _, _, _, kw, _ = E.request("categorical")
    kw.pop("condition")
    kw = E.to_device(kw, DEV)
    x = kw.pop("x")
    model = TMM.build(False, DEV)
    n = P.counters_of(K * B * E.L)
    weights = (0.3, 0.3, 2.0)
    eager = MVAEInference(model, seed=seed, use_graph=False)
    keep = lambda r: {k: v.clone() for k, v in r.items() if torch.is_tensor(v)}
    e = [keep(eager.score(x, samples=K, **dict(kw, kl_weight=w))) for w in (0.3,) + weights]
    graph = MVAEInference(model, seed=seed)
    assert graph.use_graph
    g = [keep(graph.score(x, samples=K, **dict(kw, kl_weight=w))) for w in weights]
    keys = [k for k in graph._graphs if ("samples", K) in k]
    assert len(keys) == 1 and len(graph._graphs) == 1 and keys[0][0] == "score"
    for c in range(3):
        a, b = g[c], e[c + 1]
        for k in ("means", "log_var", "kl", "ratio"):
            assert torch.equal(a[k], b[k]), (c, k)
        for k in ("bce_visual", "bce_tactile", "mse_pose", "log_w", "rows", "ess"):
            assert torch.allclose(a[k], b[k], rtol=RTOL_SUM, atol=0.0), (c, k)
    assert not torch.equal(g[0]["ratio"], g[1]["ratio"]) and not torch.equal(g[1]["ratio"], g[2]["ratio"])
    assert float((g[2]["rows"] - g[1]["rows"]).abs().min()) > 0
    for who, res, first in (("eager", e, 0), ("graph", g, 1)):
        for c, r in enumerate(res):
            want, bound = philox_ratio(r["means"].cpu(), r["log_var"].cpu(), K, seed, (c + first) * n)
            err = (r["ratio"].cpu() - want).abs()
            print(who, "call", c, "largest |ratio - philox| / bound", float((err / bound).max()))
            assert bool((err <= bound).all()), (who, c)
            other, _ = philox_ratio(r["means"].cpu(), r["log_var"].cpu(), K, seed, (c + first + 1) * n)
            assert bool(((r["ratio"].cpu() - other).abs() > bound).any())                  # (the next block is somebody else's)
    graph.close(), eager.close()


def test_score_samples_on_dirty_allocator_memory(monkeypatch):
    """score(samples=K), eager, mixed availability, with every torch.empty of ops / layers / engine pre-filled with zeros, NaNs or
    junk (tests/dirty.py) and with the real torch.empty: the same bits; the fp64 row tables and what is assembled from them come
    from atomics (rtol 1e-12)."""
    B, K, categorical, kw, eps = E.request("mixed")
    kw = E.to_device(kw, DEV)
    x = kw.pop("x")
    got = {}
    for fill in (None,) + dirty.FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else dirty.PoisonTorch(fill))
        eng = MVAEInference(TMM.build(False, DEV), use_graph=False)
        try:
            eng.noise = E.InjectedNoise([eps.clone()], [])
            r = eng.score(x, samples=K, **kw)
            torch.cuda.synchronize()
            res = {k: v.detach().cpu().clone() for k, v in r.items() if torch.is_tensor(v)}
            res.update({f"recon_x {i}": t.detach().cpu().clone() for i, t in enumerate(r["recon_x"])})
        finally:
            eng.close()
        got["real torch.empty" if fill is None else fill] = res
    dirty.assert_same_bits(got, approx=("rows", "ess", "log_w", "bce_visual", "bce_tactile", "mse_pose"), what="score(samples): ")
