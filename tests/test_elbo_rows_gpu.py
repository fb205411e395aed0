"""Per-sample ELBO on a real MI355X: every mmdyn_*_rows* entry point against an fp64 restatement and against the scalar kernel
it is the per-sample form of, the fused last decoder layer in ROWS mode against the unfused pair, MVAEStep.score_step and the
Problem API against the reference's rows (tests/golden/elbo_rows.npz) and, at the batch sizes of test_fused_engine_vs_oracle,
against a per-sample restatement built here from the CPU oracle's forward functions.

None of the cases below is shape-skipped on an MI355X: zero skips."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rows_cases as C
import test_elbo_rows_emu as TE
import test_model_emu as T
from oracle import mvae_oracle as O
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.models.shapes import state_dict_shapes
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_batch, seeded_noise
from test_kernels_aten_gpu import rel, rnd, nhwc_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
# tests/test_kernels_gpu.py::test_bce_logits_groups_masked / _equals_per_pass_launches: the sums against the fp32 CPU restatement
RTOL_SUM = 1e-5
# ... and two launches of the same element arithmetic that differ in their fp64 summation order only
RTOL_SAME = 1e-12


def f64(*shape):
    return torch.zeros(*shape, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("B,S,mask_c", [(1, 64, 0), (5, 64, 1), (37, 64, 3), (256, 64, 0), (5, 128, 1), (5, 256, 0), (2, 256, 3),
                                        (37, 128, 0)])
def test_bce_logits_rows_groups(B, S, mask_c):
    """G = 4 passes against one target: a discarded pass (slot -1) and two passes sharing a slot; odd and even batch sizes, the
    three image sizes, no mask / a 1-channel / a 3-channel mask.  Against fp64 torch per sample, and the rows of a slot add up to
    what mmdyn_bce_logits_groups[_masked] puts into that slot on the same buffers."""
    G, slots, n_slots = 4, [2, -1, 0, 2], 3
    chw, hw = 3 * S * S, S * S
    lg = rnd(G, B, chw, seed=500) * 3
    tg = torch.rand(B, chw, generator=torch.Generator().manual_seed(501))
    mk = (torch.rand(B, mask_c, hw, generator=torch.Generator().manual_seed(502)) > 0.35).float() if mask_c else None
    want, want_u = torch.zeros(n_slots, B, dtype=torch.float64), torch.zeros(n_slots, B, dtype=torch.float64)
    for g, s in enumerate(slots):
        if s < 0:
            continue
        x, t = lg[g].double(), tg.double()
        want_u[s] += F.binary_cross_entropy_with_logits(x, t, reduction="none").sum(1)
        if mk is not None:
            m = mk.double().expand(B, 3, hw).reshape(B, chw)
            x, t = x * m, t * m
        want[s] += F.binary_cross_entropy_with_logits(x, t, reduction="none").sum(1)
    lgd, tgd, mkd = lg.to(DEV), tg.to(DEV), None if mk is None else mk.to(DEV)
    rows, rows_u = f64(n_slots, B), f64(n_slots, B)
    HIP.bce_logits_rows_groups(lgd, tgd, rows, slots, B, chw, mask=mkd, hw=hw, mask_channels=max(mask_c, 1),
                               unmasked_rows=rows_u if mk is not None else None)
    torch.cuda.synchronize()
    print("bce rows", B, S, mask_c, "max rel", float(((rows.cpu() - want).abs() / want.abs().clamp_min(1e-30)).max()))
    assert torch.allclose(rows.cpu(), want, rtol=RTOL_SUM)
    assert float(rows[1].abs().max()) == 0.0                    # no pass writes slot 1
    if mk is not None:
        assert torch.allclose(rows_u.cpu(), want_u, rtol=RTOL_SUM)
    loss, un = f64(8), f64(8)
    kw = {} if mk is None else dict(mask=mkd, chw=chw, hw=hw, mask_channels=mask_c, unmasked_slots=un)
    HIP.bce_logits_groups(lgd, tgd, None, loss, slots, B * chw, 1.0, **kw)
    assert torch.allclose(rows.sum(1).cpu(), loss[:n_slots].cpu(), rtol=RTOL_SAME)
    if mk is not None:
        assert torch.allclose(rows_u.sum(1).cpu(), un[:n_slots].cpu(), rtol=RTOL_SAME)
    # host-side checks: a slot beyond the table, a table of the wrong batch, a mask of the wrong size
    with pytest.raises(ops._lib.MmdynError):
        HIP.bce_logits_rows_groups(lgd, tgd, rows, [3, 0, 0, 0], B, chw)
    with pytest.raises(ValueError):
        HIP.bce_logits_rows_groups(lgd, tgd, f64(n_slots, B + 1), slots, B, chw)
    if mk is not None:
        with pytest.raises(ValueError):
            HIP.bce_logits_rows_groups(lgd, tgd, rows, slots, B, chw, mask=mkd.reshape(-1)[:-4], hw=hw, mask_channels=mask_c)


@pytest.mark.parametrize("B", [1, 5, 37, 256])
def test_mse_rows_groups_kl_rows_and_assembly(B):
    """mmdyn_mse_rows_groups (two passes sharing a slot), mmdyn_kl_rows and mmdyn_elbo_assemble_rows (both KL modes, the KL weight
    from device memory) against fp64 torch, and the row sums against mmdyn_mse_groups / the kl_sum of mmdyn_reparam_fwd."""
    G, slots, n_slots, n = 3, [1, 0, 1], 2, 7
    r, t = rnd(G, B, n, seed=510), torch.rand(B, n, generator=torch.Generator().manual_seed(511))
    want = torch.zeros(n_slots, B, dtype=torch.float64)
    for g, s in enumerate(slots):
        want[s] += ((r[g].double() - t.double()) ** 2).sum(1)
    rd, td = r.to(DEV), t.to(DEV)
    rows = f64(n_slots, B)
    HIP.mse_rows_groups(rd, td, rows, slots, B, n)
    assert torch.allclose(rows.cpu(), want, rtol=RTOL_SUM)
    loss = f64(8)
    HIP.mse_groups(rd, td, None, loss, slots, B * n, 1.0)
    assert torch.allclose(rows.sum(1).cpu(), loss[:n_slots].cpu(), rtol=RTOL_SAME)
    with pytest.raises(ops._lib.MmdynError):
        HIP.mse_rows_groups(rd, td, rows, [1, -1, 0], B, n)
    # KL rows of P = 3 passes
    P, L = 3, 256
    mu, lv = rnd(P, B, L, seed=512), rnd(P, B, L, seed=513) * 2 - 1
    want_kl = -0.5 * (1 + lv.double() - mu.double() ** 2 - lv.double().exp()).sum(2)
    mud, lvd = mu.to(DEV), lv.to(DEV)
    kl_rows, kl_sum = f64(P, B), f64(P)
    HIP.kl_rows(mud, lvd, kl_rows, P, B, L)
    assert torch.allclose(kl_rows.cpu(), want_kl, rtol=RTOL_SUM)
    for p in range(P):
        HIP.reparam_fwd(mud[p], lvd[p], None, None, kl_sum[p:p + 1], B, L, L)
    print("kl rows", B, "sum vs kl_sum", float(((kl_rows.sum(1) - kl_sum).abs() / kl_sum.abs()).max()))
    assert torch.allclose(kl_rows.sum(1).cpu(), kl_sum.cpu(), rtol=RTOL_SAME)
    # assembly
    bce = torch.rand(P, B, dtype=torch.float64, generator=torch.Generator().manual_seed(514)) * 9000
    mse = torch.rand(P, B, dtype=torch.float64, generator=torch.Generator().manual_seed(515))
    klw_arg, klw_dev, pm = 0.5, 0.04, 1000.0
    for mode in (0, 1):
        kl = kl_rows.cpu() if mode else kl_sum.cpu().reshape(P, 1).expand(P, B)
        want_p = bce + pm * mse + klw_arg * klw_dev * kl
        out, partials = torch.empty(B, device=DEV), torch.empty(P, B, device=DEV)
        HIP.elbo_assemble_rows(bce.to(DEV), mse.to(DEV), kl_rows, kl_sum, out, partials, P, B, klw_arg, pm,
                               kl_weight_dev=torch.tensor([klw_dev], device=DEV), kl_mode=mode)
        assert torch.allclose(partials.double().cpu(), want_p, rtol=1e-6)
        assert torch.allclose(out.double().cpu(), want_p.sum(0), rtol=1e-6)
    out = torch.empty(B, device=DEV)
    HIP.elbo_assemble_rows(bce.to(DEV), None, None, None, out, None, P, B, 1.0, pm)
    assert torch.allclose(out.double().cpu(), bce.sum(0), rtol=1e-6)


@pytest.mark.parametrize("G,Bg,H,dtype,mask_c,keep", [(4, 3, 32, torch.float32, 0, 1), (2, 2, 32, torch.float32, 1, -1), (3, 2, 32, torch.float32, 3, 0),
                                                      (4, 5, 32, torch.bfloat16, 0, 3), (2, 1, 64, torch.float16, 1, None), (1, 2, 128, torch.float32, 0, 0)])
def test_last_decoder_layer_with_the_loss_rows_in_its_epilogue(G, Bg, H, dtype, mask_c, keep):
    """mmdyn_tconv_out3_bn_bce_rows against the unfused pair (mmdyn_tconv_out3_bn_fwd, then mmdyn_bce_logits_rows_groups on the
    written logits) on the same inputs -- the cases and bounds of test_last_decoder_layer_with_the_loss_in_its_epilogue: the row sums
    to fp32 summation order (1e-7), the published logits bit for bit -- and against fp64 ATen (2e-6); the rows of a slot add up to the
    slot of the scalar fused launch."""
    B, S = G * Bg, 2 * H
    prec = {torch.float32: "fp32", torch.bfloat16: "bf16s", torch.float16: "fp16s"}[dtype]
    y = (rnd(B, 32, H, H, seed=60) * 2 + 0.3).to(dtype)
    mean, rstd = rnd(G, 32, seed=61) * 0.3, rnd(G, 32, seed=62).abs() + 0.5
    gamma, beta = rnd(32, seed=63) + 1.2, rnd(32, seed=64)
    W = rnd(32, 3, 4, 4, seed=65, scale=0.2)
    g = torch.Generator().manual_seed(66)
    target = torch.rand(Bg, 3, S, S, generator=g)
    mask = (torch.rand(Bg, mask_c, S, S, generator=g) > 0.3).float() if mask_c else None
    slots = [5, -1, 0, 2][:G] if G > 1 else [1]
    n_slots = 8
    yd = y.double()
    xh = (yd.reshape(G, Bg, 32, H, H) - mean.double().reshape(G, 1, 32, 1, 1)) * rstd.double().reshape(G, 1, 32, 1, 1)
    u = (xh * gamma.double().reshape(1, 1, 32, 1, 1) + beta.double().reshape(1, 1, 32, 1, 1)).reshape(B, 32, H, H)
    lg = F.conv_transpose2d(u * torch.sigmoid(u), W.double(), stride=2, padding=1).reshape(G, Bg, 3, S, S)
    md = None if mask is None else mask.double()
    want, want_u = torch.zeros(n_slots, Bg, dtype=torch.float64), torch.zeros(n_slots, Bg, dtype=torch.float64)
    for gi, sl in enumerate(slots):
        if sl < 0:
            continue
        a, t = (lg[gi], target.double()) if md is None else (lg[gi] * md, target.double() * md)
        want[sl] += F.binary_cross_entropy_with_logits(a, t, reduction="none").sum((1, 2, 3))
        want_u[sl] += F.binary_cross_entropy_with_logits(lg[gi], target.double(), reduction="none").sum((1, 2, 3))
    prev = ops.B.precision
    ops.B.precision = prec
    try:
        args = (nhwc_rows(y).to(DEV), mean.to(DEV), rstd.to(DEV), gamma.to(DEV), beta.to(DEV), W.to(DEV))
        mkd = None if mask is None else mask.to(DEV)
        rows, rows_u = f64(n_slots, Bg), f64(n_slots, Bg)
        out = None if keep is None else torch.full((B if keep < 0 else Bg, 3, S, S), 7.0, device=DEV)
        ops.B.tconv_out3_bn_bce_rows(*args, out, -1 if keep is None else keep, target.to(DEV), rows, slots, G, Bg, H, H, mask=mkd,
                                     mask_channels=max(mask_c, 1), unmasked_rows=rows_u if mask is not None else None)
        print("fused rows", G, Bg, H, dtype, "vs fp64", rel(rows, want))
        assert rel(rows, want) < 2e-6 and (mask is None or rel(rows_u, want_u) < 2e-6)
        # the unfused pair
        out2 = torch.empty(B, 3, S, S, device=DEV)
        rows2, rows2_u = f64(n_slots, Bg), f64(n_slots, Bg)
        ops.B.tconv_out3_bn_fwd(*args, out2, G, Bg, H, H)
        ops.B.bce_logits_rows_groups(out2, target.to(DEV), rows2, slots, Bg, 3 * S * S, mask=mkd, hw=S * S,
                                     mask_channels=max(mask_c, 1), unmasked_rows=rows2_u if mask is not None else None)
        assert rel(rows, rows2) < 1e-7 and (mask is None or rel(rows_u, rows2_u) < 1e-7)
        if keep is not None:
            assert torch.equal(out, out2 if keep < 0 else out2[keep * Bg:(keep + 1) * Bg])
        # the scalar fused launch on the same buffers
        acc, acc_u = f64(n_slots), f64(n_slots)
        ops.B.tconv_out3_bn_bce(*args, None, -1, target.to(DEV), None, acc, slots, 1.0, G, Bg, H, H, mask=mkd,
                                mask_channels=max(mask_c, 1), unmasked_slots=acc_u if mask is not None else None)
        assert torch.allclose(rows.sum(1).cpu(), acc.cpu(), rtol=RTOL_SAME)
        if mask is not None:
            assert torch.allclose(rows_u.sum(1).cpu(), acc_u.cpu(), rtol=RTOL_SAME)
    finally:
        ops.B.precision = prev


@pytest.mark.parametrize("name", list(C.MVAE_CASES))
def test_mvae_rows_module_api(golden_dir, name):
    TE.check_mvae_rows_module_api(golden_dir, DEV, name)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
@pytest.mark.parametrize("name", list(C.MVAE_CASES))
def test_mvae_rows_fused_engine(golden_dir, name, precision):
    TE.check_mvae_rows_engine(golden_dir, DEV, name, precision)


@pytest.mark.parametrize("name", list(C.VAE_CASES))
def test_vae_rows(golden_dir, name):
    TE.check_vae_rows(golden_dir, DEV, name)


def test_problem_score(golden_dir):
    g = T.load(golden_dir, "elbo_rows.npz")
    for r in TE.check_score_wrapper(DEV).values():
        np.testing.assert_allclose(r.cpu().numpy(), g["pose/rows"], rtol=TE.REL)


def oracle_rows(prm, buf, inputs, targets, eps, masks, klw, use_pose, loss_mask=None, pm=1000.0):
    """Per-sample restatement on the CPU oracle's forward: for every subset pass one O.mvae_forward, then the per-sample BCE / MSE /
    KL of that pass.  -> (bce [P][B], mse [P][B], kl [P][B]) in fp64."""
    subsets = O.SUBSETS_POSE if use_pose else O.SUBSETS_NOPOSE
    v, t = inputs[0], inputs[1]
    p = inputs[2] if use_pose else None
    mask_it = iter(masks)
    bce, mse, kl = [], [], []
    with torch.no_grad():
        for i, (a, b, c) in enumerate(subsets):
            vr, tr, pr, mu, lv = O.mvae_forward(prm, v if a else None, t if b else None, p if c else None, eps[i], mask_it, use_pose, buf)
            e = torch.zeros(v.shape[0], dtype=torch.float64)
            for on, r, x in ((a, vr, targets[0]), (b, tr, targets[1])):
                if on:
                    r, x = r.double(), x.double()
                    if loss_mask is not None:
                        r, x = r * loss_mask.double(), x * loss_mask.double()
                    e = e + F.binary_cross_entropy_with_logits(r, x, reduction="none").sum((1, 2, 3))
            bce.append(e)
            mse.append(((pr.double() - targets[2].double()) ** 2).sum(1) if c else torch.zeros_like(e))
            kl.append(-0.5 * (1 + lv.double() - mu.double() ** 2 - lv.double().exp()).sum(1))
    return torch.stack(bce), torch.stack(mse), torch.stack(kl)


@pytest.mark.parametrize("B,use_pose,masked", [(256, True, False), (130, True, False), (37, True, False), (5, True, False), (1, True, False),
                                               (37, False, False), (5, False, True), (256, False, True)])
def test_score_step_vs_oracle(B, use_pose, masked):
    """score_step in the default arithmetic at the batch sizes of test_fused_engine_vs_oracle against the per-sample restatement
    above, both KL modes, at that test's bound on the loss (1e-4 relative); and the identities: rows(kl="sample").sum() / B is
    eval_step's scalar, rows("batch") - rows("sample") = kl_weight * sum over passes of (kl_sum - kl_rows), the KL rows add up to
    the kl_sum of mmdyn_poe_fwd."""
    klw, pm = 1.0 / 50, 1000.0
    sd = seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=use_pose), 0)
    prm, buf = O.split_state(sd)
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass, n_mask, 4321)
    lm = C.loss_mask(B, 1) if masked else None
    bce, mse, kl = oracle_rows(prm, buf, inputs, targets, eps, masks, klw, use_pose, lm)
    step = MVAEStep(T.build("cnn-mvae", True, use_pose, DEV), pose_multiplier=pm)
    assert step.precision == "fp32x3"
    gi, gt = [x.to(DEV) for x in inputs], [x.to(DEV) for x in targets]
    lmd = None if lm is None else lm.to(DEV)
    res = {}
    for mode in ("batch", "sample"):
        step.noise = InjectedNoise(list(eps), list(masks))
        res[mode] = step.score_step(gi, gt, klw, loss_mask=lmd, kl=mode)
    step.noise = InjectedNoise(list(eps), list(masks))
    ev = float(step.eval_step(gi, gt, klw, loss_mask=lmd))
    want = {"sample": bce + pm * mse + klw * kl, "batch": bce + pm * mse + klw * kl.sum(1, keepdim=True)}
    for mode in ("batch", "sample"):
        got = res[mode]
        err = float(((got["rows"].double().cpu() - want[mode].sum(0)).abs() / want[mode].sum(0).abs()).max())
        print("score_step", B, use_pose, masked, mode, "max rel row error", err)
        np.testing.assert_allclose(got["rows"].double().cpu().numpy(), want[mode].sum(0).numpy(), rtol=1e-4)
        np.testing.assert_allclose(got["partials"].double().cpu().numpy(), want[mode].numpy(), rtol=1e-4)
    rb, rs = res["batch"], res["sample"]
    assert float(rb["loss"]) == pytest.approx(ev, rel=1e-6)
    assert float(rs["rows"].double().sum()) / B == pytest.approx(ev, rel=1e-5)
    klr = rb["kl_rows"]
    assert torch.allclose(klr.sum(1).cpu(), step.acc[2][:n_pass].cpu(), rtol=RTOL_SAME)
    diff = (rb["rows"].double() - rs["rows"].double()).cpu()
    want_d = (klw * (klr.sum(1, keepdim=True) - klr)).sum(0).cpu()
    np.testing.assert_allclose(diff.numpy(), want_d.numpy(), rtol=1e-3, atol=0.05)       # (fp32 rows of ~1e5: half an ulp is 4e-3)
    step.close()


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_inference_score(golden_dir, precision):
    TE.check_inference_score(golden_dir, DEV, precision)


def test_inference_score_replay_gives_each_input_its_own_rows():
    """The captured score graph: two calls with DIFFERENT inputs of one shape give each input's own terms (the deterministic ones
    -- the KL rows depend on the inputs only -- equal to the eager engine's bit for bit, the reconstruction terms equal to torch on
    the logits the call returned), the KL weight is read at replay time, and close() drops the graphs."""
    B = 5
    a_in, a_tg = seeded_batch(B, 101)
    b_in, b_tg = seeded_batch(B, 202)
    a_in, a_tg, b_in, b_tg = ([x.to(DEV) for x in l] for l in (a_in, a_tg, b_in, b_tg))
    eng = TE.eval_engine(DEV, seed=5)
    eager = TE.eval_engine(DEV, seed=5)
    eager.use_graph = False
    got = {}
    for name, (i, t), klw in (("a", (a_in, a_tg), 0.5), ("b", (b_in, b_tg), 0.5), ("a2", (a_in, a_tg), 2.0)):
        r = eng.score([i[0], i[1]], pose=i[2], targets=t, kl_weight=klw)
        bv = F.binary_cross_entropy_with_logits(r["recon_x"][0].double(), t[0].double(), reduction="none").sum((1, 2, 3))
        bt = F.binary_cross_entropy_with_logits(r["recon_x"][1].double(), t[1].double(), reduction="none").sum((1, 2, 3))
        mp = ((r["recon_x"][2].double() - t[2].double()) ** 2).sum(1)
        assert torch.allclose(r["bce_visual"], bv, rtol=RTOL_SUM) and torch.allclose(r["bce_tactile"], bt, rtol=RTOL_SUM)
        assert torch.allclose(r["mse_pose"], mp, rtol=RTOL_SUM)
        assert torch.allclose(r["rows"].double(), bv + bt + 1000.0 * mp + klw * r["kl"], rtol=1e-6)
        e = eager.score([i[0], i[1]], pose=i[2], targets=t, kl_weight=klw)
        assert torch.equal(r["kl"], e["kl"]) and torch.equal(r["means"], e["means"])
        got[name] = {k: r[k].clone() for k in ("kl", "bce_visual", "rows")}
    assert len([k for k in eng._graphs if k[0] == "score"]) == 1            # one capture served the three calls
    assert not torch.equal(got["a"]["kl"], got["b"]["kl"]) and torch.equal(got["a"]["kl"], got["a2"]["kl"])
    assert float((got["a"]["bce_visual"] - got["b"]["bce_visual"]).abs().min()) > 0
    eng.close()
    assert eng._graphs == {}
    eager.close()


def test_row_entry_points_reject_bad_arguments():
    """Null pointers and slot ranges are refused on the host, before any launch, by every new entry point."""
    lib = HIP.lib
    assert lib.mmdyn_bce_logits_rows_groups(None, None, None, 1, None, None, None, 1, 1, 1, 4, 4, None) == -2
    assert lib.mmdyn_kl_rows(None, None, None, 1, 1, 1, None) == -2
    assert lib.mmdyn_elbo_assemble_rows(None, None, None, None, None, None, 1, 1, 1.0, 1.0, None, 0, None) == -2
    assert lib.mmdyn_mse_rows_groups(None, None, None, None, 1, 1, 1, 7, None) == -2
    assert lib.mmdyn_tconv_out3_bn_bce_rows(None, None, None, None, None, None, None, -1, None, None, 1, None, None, None, 1, 1, 1, 16,
                                            16, 0, None) == -2
    G, Bg, H = 2, 2, 16
    y = torch.zeros(G * Bg * H * H, 32, device=DEV)
    st, w = torch.ones(G, 32, device=DEV), torch.zeros(32, 3, 4, 4, device=DEV)
    tg, rows = torch.zeros(Bg, 3, 2 * H, 2 * H, device=DEV), f64(2, Bg)
    args = (y, st, st, st[0], st[0], w, None, -1, tg, rows)
    with pytest.raises(ops._lib.MmdynError):                     # a slot at the end of the table
        HIP.tconv_out3_bn_bce_rows(*args, [0, 2], G, Bg, H, H)
    with pytest.raises(ValueError):                              # a table of another batch size
        HIP.tconv_out3_bn_bce_rows(*args[:-1], f64(2, Bg + 1), [0, 1], G, Bg, H, H)
    with pytest.raises(ops._lib.MmdynError):                     # kl_mode outside {0, 1}
        HIP.elbo_assemble_rows(rows, None, None, None, torch.zeros(Bg, device=DEV), None, 2, Bg, 1.0, 1.0, kl_mode=2)
    HIP.tconv_out3_bn_bce_rows(*args, [0, -1], G, Bg, H, H)      # (the accepted form of the same call)
    torch.cuda.synchronize()
    assert float(rows[1].abs().max()) == 0.0 and float(rows[0].min()) > 0
