"""Per-sample weights in training on a real MI355X: every weighted entry point against its unweighted sibling (w = 1: bit for bit),
against the w-scaling it promises (each sample's gradient block = the w = 1 block times w_b, recomputed in fp32, bitwise) and
against fp64 torch, with guard regions around the outputs; MVAEStep / the module API / Problem.train_batch against the reference
fixture (tests/golden/weighted_elbo.npz) and the oracle restatement of tests/test_weighted_emu.py; graph replay.

Run-to-run repeatability of the UNWEIGHTED eager step is measured first (test_ones_equals_unweighted_step prints it): where two such
steps agree bitwise the weighted step with w = 1 must equal them bitwise, otherwise the bound is four times the measured difference
(docs/LAB_NOTES.md M)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rows_cases as C
import test_model_emu as T
import test_weighted_emu as TW
import weighted_cases as W
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.models.vae import NoiseSource
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise
from test_kernels_aten_gpu import rel, rnd, nhwc_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
GUARD = 64            # floats of guard band on either side of a gradient output
MAGIC = 12345.0


def f64(*shape):
    return torch.zeros(*shape, dtype=torch.float64, device=DEV)


def guarded(n):
    """(whole buffer, the n-element output view in its middle); the bands hold MAGIC."""
    buf = torch.full((n + 2 * GUARD,), MAGIC, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool((buf[:GUARD] == MAGIC).all()) and bool((buf[-GUARD:] == MAGIC).all())


def scaled_rows(d1, w, G, Bg):
    """The w = 1 gradient [G][Bg][...] times w_b in fp32 (one multiplication per element: what the kernels promise bitwise)."""
    v = d1.reshape(G, Bg, -1)
    return (v * w.reshape(1, Bg, 1)).reshape(-1)


@pytest.mark.parametrize("B,mask_c", [(1, 0), (5, 1), (37, 3), (37, 0)])
def test_bce_logits_rows_groups_grad(B, mask_c):
    G, slots, n_slots, S = 4, [2, -1, 0, 2], 3, 64
    chw, hw = 3 * S * S, S * S
    lg = (rnd(G, B, chw, seed=700) * 3).to(DEV)
    tg = torch.rand(B, chw, generator=torch.Generator().manual_seed(701)).to(DEV)
    mk = (torch.rand(B, mask_c, hw, generator=torch.Generator().manual_seed(702)) > 0.35).float().to(DEV) if mask_c else None
    gs = 0.37
    kw = dict(mask=mk, hw=hw if mask_c else 0, mask_channels=max(mask_c, 1))
    # the siblings: rows from the rows kernel, the gradient from the scalar kernel
    rows0, rows0_u = f64(n_slots, B), f64(n_slots, B)
    HIP.bce_logits_rows_groups(lg, tg, rows0, slots, B, chw, unmasked_rows=rows0_u if mask_c else None, **kw)
    d0 = torch.empty_like(lg)
    skw = {} if mk is None else dict(mask=mk, chw=chw, hw=hw, mask_channels=mask_c, unmasked_slots=f64(8))
    HIP.bce_logits_groups(lg, tg, d0, f64(8), slots, B * chw, gs, **skw)
    # w = 1
    ones = torch.ones(B, device=DEV)
    buf, d1 = guarded(lg.numel())
    rows1, rows1_u = f64(n_slots, B), f64(n_slots, B)
    HIP.bce_logits_rows_groups_grad(lg, tg, d1, ones, rows1, slots, B, chw, gs, unmasked_rows=rows1_u if mask_c else None, **kw)
    torch.cuda.synchronize()
    assert torch.equal(d1, d0.reshape(-1)) and guards_intact(buf)
    assert torch.allclose(rows1, rows0, rtol=1e-12) and (not mask_c or torch.allclose(rows1_u, rows0_u, rtol=1e-12))
    assert float(d1.reshape(G, -1)[1].abs().max()) == 0.0          # the discarded pass
    # random weights: mixed magnitudes, a zero, a negative one
    w = W.weights(B).to(DEV)
    buf, d2 = guarded(lg.numel())
    rows2 = f64(n_slots, B)
    HIP.bce_logits_rows_groups_grad(lg, tg, d2, w, rows2, slots, B, chw, gs, **kw)
    torch.cuda.synchronize()
    assert torch.equal(d2, scaled_rows(d1, w, G, B)) and guards_intact(buf)
    assert torch.equal(rows2, rows1) or torch.allclose(rows2, rows1, rtol=1e-12)      # the sums are not weighted
    # fp64 torch
    x, t = lg.double().reshape(G, B, chw), tg.double()
    m = 1.0 if mk is None else mk.double().expand(B, 3, hw).reshape(B, chw)
    want = (m * (torch.sigmoid(x * m) - t * m) * gs) * w.double().reshape(1, B, 1)
    want[1] = 0
    assert rel(d2.reshape(G, B, chw), want) < 2e-6
    # bad arguments
    with pytest.raises(ops._lib.MmdynError):
        HIP.bce_logits_rows_groups_grad(lg, tg, d2, w, rows2, [3, 0, 0, 0], B, chw, gs)
    with pytest.raises(ValueError):
        HIP.bce_logits_rows_groups_grad(lg, tg, d2, w[:-1] if B > 1 else torch.ones(2, device=DEV), rows2, slots, B, chw, gs)
    with pytest.raises(ValueError):
        HIP.bce_logits_rows_groups_grad(lg, tg, d2[:-4], w, rows2, slots, B, chw, gs)
    lib = HIP.lib
    assert lib.mmdyn_bce_logits_rows_groups_grad(None, None, None, 1, None, None, None, None, None, 1, 1.0, 1, 1, 4, 4, None) == -2


@pytest.mark.parametrize("B", [1, 5, 37])
def test_mse_rows_groups_grad(B):
    G, slots, n_slots, n, gs = 3, [1, 0, 1], 2, 7, 250.0
    r = rnd(G, B, n, seed=710).to(DEV)
    t = torch.rand(B, n, generator=torch.Generator().manual_seed(711)).to(DEV)
    rows0, d0 = f64(n_slots, B), torch.empty_like(r)
    HIP.mse_rows_groups(r, t, rows0, slots, B, n)
    HIP.mse_groups(r, t, d0, f64(8), slots, B * n, gs)
    buf, d1 = guarded(r.numel())
    rows1 = f64(n_slots, B)
    HIP.mse_rows_groups_grad(r, t, d1, torch.ones(B, device=DEV), rows1, slots, B, n, gs)
    torch.cuda.synchronize()
    assert torch.equal(d1, d0.reshape(-1)) and guards_intact(buf) and torch.allclose(rows1, rows0, rtol=1e-12)
    w = W.weights(B).to(DEV)
    buf, d2 = guarded(r.numel())
    HIP.mse_rows_groups_grad(r, t, d2, w, f64(n_slots, B), slots, B, n, gs)
    torch.cuda.synchronize()
    assert torch.equal(d2, scaled_rows(d1, w, G, B)) and guards_intact(buf)
    want = (2 * (r.double() - t.double().reshape(1, B, n)) * gs) * w.double().reshape(1, B, 1)
    assert rel(d2.reshape(G, B, n), want) < 2e-6
    with pytest.raises(ops._lib.MmdynError):
        HIP.mse_rows_groups_grad(r, t, d2, w, f64(n_slots, B), [1, -1, 0], B, n, gs)
    with pytest.raises(ops._lib.MmdynError):
        HIP.mse_rows_groups_grad(r, t, d2, w, f64(n_slots, B), [2, 0, 0], B, n, gs)
    assert HIP.lib.mmdyn_mse_rows_groups_grad(None, None, None, None, None, None, 1, 1.0, 1, 1, 7, None) == -2


def _poe_setup(P, B, L, seed):
    """P passes over three experts (some absent), heads [B][2L] per expert, decoder latent gradients for some passes."""
    heads = [(rnd(B, 2 * L, seed=seed + m) * 0.7).to(DEV) for m in range(3)]
    subsets = [(1, 1, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1)][:P]
    eps = rnd(P, B, L, seed=seed + 9).to(DEV)
    dzs = [[(rnd(B, L, seed=seed + 20 + 3 * p + k) * 0.1).to(DEV) if (k < 2 and s[k]) else None for k in range(3)]
           for p, s in enumerate(subsets)]

    def passes(dheads):
        out = []
        for p, s in enumerate(subsets):
            hs = [heads[m] if s[m] else None for m in range(3)]
            ds = [dheads[p][m] if s[m] else None for m in range(3)]
            out.append({"mu": [None if h is None else h[:, :L] for h in hs], "lv": [None if h is None else h[:, L:] for h in hs],
                        "dmu": [None if d is None else d[:, :L] for d in ds], "dlv": [None if d is None else d[:, L:] for d in ds],
                        "ld": [2 * L] * 3, "dz": dzs[p]})
        return out
    return heads, subsets, eps, passes


@pytest.mark.parametrize("B", [1, 5, 37, 256])
def test_poe_bwd_weighted(B):
    P, L, ks = 7, 256, 0.013
    heads, subsets, eps, passes = _poe_setup(P, B, L, 720)
    mu, lv = torch.empty(P, B, L, device=DEV), torch.empty(P, B, L, device=DEV)
    HIP.poe_fwd(passes([[None] * 3] * P), eps, mu, lv, torch.empty(P, B, L, device=DEV), None, True, P, B, L)
    klw = torch.tensor([0.6], device=DEV)

    def run(w):
        bufs = [[guarded(B * 2 * L) for _ in range(3)] for _ in range(P)]
        dh = [[b[1].view(B, 2 * L) for b in row] for row in bufs]
        if w is None:
            HIP.poe_bwd(passes(dh), eps, mu, lv, None, None, None, ks, True, P, B, L, klw)
        else:
            HIP.poe_bwd_weighted(passes(dh), eps, mu, lv, None, None, None, ks, w, True, P, B, L, klw)
        torch.cuda.synchronize()
        assert all(guards_intact(b[0]) for row in bufs for b in row)
        return [[dh[p][m] if subsets[p][m] else None for m in range(3)] for p in range(P)]

    d0, d1 = run(None), run(torch.ones(B, device=DEV))
    for p in range(P):
        for m in range(3):
            if subsets[p][m]:
                assert torch.equal(d1[p][m], d0[p][m]), (p, m)
    # fp64 autograd with a per-row KL scale
    w = W.weights(B).to(DEV)
    d2 = run(w)
    eps_p = 1e-8
    for p, s in enumerate(subsets):
        hs = [heads[m].double().clone().requires_grad_(True) if s[m] else None for m in range(3)]
        sumT = torch.ones(B, L, dtype=torch.float64, device=DEV) / (1.0 + 2 * eps_p)
        sumMuT = torch.zeros(B, L, dtype=torch.float64, device=DEV)
        for h in hs:
            if h is not None:
                T_ = 1.0 / (torch.exp(h[:, L:]) + 2 * eps_p)
                sumT, sumMuT = sumT + T_, sumMuT + h[:, :L] * T_
        pm, plv = sumMuT / sumT, torch.log(1.0 / sumT + eps_p)
        obj = ((ks * 0.6 * w.double())[:, None] * (-0.5 * (1 + plv - pm * pm - plv.exp()))).sum()
        gz = sum(t.double() for t in passes([[None] * 3] * P)[p]["dz"] if t is not None) if any(s[:2]) else None
        if gz is not None:
            obj = obj + ((eps[p].double() * torch.exp(0.5 * plv) + pm) * gz).sum()
        obj.backward()
        for m in range(3):
            if s[m]:
                assert rel(d2[p][m], hs[m].grad) < 1e-4, (p, m, rel(d2[p][m], hs[m].grad))
    assert HIP.lib.mmdyn_poe_bwd_weighted(None, None, None, None, None, None, None, 1.0, None, 1, 1, 1, 1, None, None) == -2
    with pytest.raises(ValueError):
        HIP.poe_bwd_weighted(passes([[torch.empty(B, 2 * L, device=DEV)] * 3] * P), eps, mu, lv, None, None, None, ks,
                             torch.ones(B + 1, device=DEV), True, P, B, L, klw)


@pytest.mark.parametrize("B", [1, 5, 37, 256])
def test_reparam_bwd_weighted(B):
    L, ks = 256, 0.21
    m, v = (rnd(B, L, seed=730) * 0.8).to(DEV), (rnd(B, L, seed=731) * 0.5).to(DEV)
    eps, dz = rnd(B, L, seed=732).to(DEV), (rnd(B, L, seed=733) * 0.1).to(DEV)
    for with_dz in (True, False):
        e_, z_ = (eps, dz) if with_dz else (None, None)
        dm0, dv0 = torch.empty_like(m), torch.empty_like(v)
        HIP.reparam_bwd(m, v, e_, z_, ks, dm0, dv0, B, L, L)
        bm, dm1 = guarded(B * L)
        bv, dv1 = guarded(B * L)
        HIP.reparam_bwd_weighted(m, v, e_, z_, ks, torch.ones(B, device=DEV), dm1.view(B, L), dv1.view(B, L), B, L, L)
        torch.cuda.synchronize()
        assert torch.equal(dm1.view(B, L), dm0) and torch.equal(dv1.view(B, L), dv0) and guards_intact(bm) and guards_intact(bv)
        w = W.weights(B).to(DEV)
        dm2, dv2 = torch.empty_like(m), torch.empty_like(v)
        HIP.reparam_bwd_weighted(m, v, e_, z_, ks, w, dm2, dv2, B, L, L)
        s = (ks * w.double())[:, None]
        want_m = s * m.double() + (dz.double() if with_dz else 0)
        want_v = -0.5 * s * (1 - v.double().exp()) + (dz.double() * eps.double() * 0.5 * torch.exp(0.5 * v.double()) if with_dz else 0)
        assert rel(dm2, want_m) < 2e-6 and rel(dv2, want_v) < 2e-6
        if not with_dz:          # no dz term: the whole gradient is the KL term, so it scales with w bitwise
            assert torch.equal(dm2, (ks * w)[:, None] * m)
    assert HIP.lib.mmdyn_reparam_bwd_weighted(None, None, None, None, 1.0, None, None, None, 1, 1, 1, None) == -2
    assert HIP.lib.mmdyn_reparam_bwd_weighted(m.data_ptr(), v.data_ptr(), None, None, 1.0, m.data_ptr(), m.data_ptr(), v.data_ptr(),
                                              B, L, L - 1, None) == -1


@pytest.mark.parametrize("B", [1, 5, 37, 256, 1000])
def test_elbo_assemble_weighted(B):
    """Both KL modes against fp64 torch; the unweighted outputs equal mmdyn_elbo_assemble_rows's bitwise; two runs agree bitwise."""
    P, pm, klw_arg, klw_dev = 7, 1000.0, 0.5, 0.04
    gen = torch.Generator().manual_seed(740 + B)
    bce = (torch.rand(P, B, dtype=torch.float64, generator=gen) * 9000).to(DEV)
    mse = torch.rand(P, B, dtype=torch.float64, generator=gen).to(DEV)
    klr = (torch.rand(P, B, dtype=torch.float64, generator=gen) * 40).to(DEV)
    kls = klr.sum(1)
    w = W.weights(B).to(DEV)
    kd = torch.tensor([klw_dev], device=DEV)
    for mode in (0, 1):
        res = []
        for rep in range(2):
            lbuf, loss = guarded(1)
            pbuf, wp = guarded(P)
            obuf, out = guarded(B)
            qbuf, parts = guarded(P * B)
            sbuf, ws = guarded(B)
            HIP.elbo_assemble_weighted(bce, mse, klr, kls, w, loss, wp, out, parts, ws, P, B, klw_arg, pm, kd, mode)
            torch.cuda.synchronize()
            assert all(guards_intact(b) for b in (lbuf, pbuf, obuf, qbuf, sbuf))
            res.append((loss.clone(), wp.clone(), out.clone(), parts.clone(), ws.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*res))
        loss, wp, out, parts, ws = res[0]
        out0, parts0 = torch.empty(B, device=DEV), torch.empty(P, B, device=DEV)
        HIP.elbo_assemble_rows(bce, mse, klr, kls, out0, parts0, P, B, klw_arg, pm, kd, mode)
        assert torch.equal(out, out0) and torch.equal(parts, parts0.reshape(-1))
        wd = w.double()
        kl = (klr * wd).sum(1) if mode else wd.sum() * kls
        want = (((bce + pm * mse) * wd).sum(1) + klw_arg * klw_dev * kl) / B
        assert torch.allclose(wp.double(), want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
        assert float(loss) == pytest.approx(float(want.sum()), rel=1e-6, abs=1e-6 * float(want.abs().max()))
        assert torch.allclose(ws, torch.full((B,), float(wd.sum()), device=DEV), rtol=1e-6) and len(set(ws.tolist())) == 1
    assert HIP.lib.mmdyn_elbo_assemble_weighted(None, None, None, None, None, None, None, None, None, None, 1, 1, 1.0, 1.0, None, 0,
                                                None) == -2
    lw = torch.empty(1, device=DEV)
    assert HIP.lib.mmdyn_elbo_assemble_weighted(None, None, None, None, w.data_ptr(), lw.data_ptr(), None, None, None, None, 9, B, 1.0,
                                                1.0, None, 0, None) == -1
    assert HIP.lib.mmdyn_elbo_assemble_weighted(None, None, None, None, w.data_ptr(), lw.data_ptr(), None, None, None, None, P, B, 1.0,
                                                1.0, None, 2, None) == -1


@pytest.mark.parametrize("G,Bg,H,dtype,mask_c,slots", [(4, 3, 32, torch.float32, 0, [5, 1, 0, 2]), (2, 2, 32, torch.float32, 1, [0, 1]),
                                                       (3, 2, 32, torch.float32, 3, [2, 0, 2]), (4, 5, 32, torch.bfloat16, 0, [0, 1, 2, 3]),
                                                       (4, 3, 32, torch.float32, 0, [5, -1, 0, 2]), (2, 1, 64, torch.float16, 1, [1, 0]),
                                                       (1, 2, 128, torch.float32, 0, [1])])
def test_last_decoder_layer_rows_and_weighted_gradient(G, Bg, H, dtype, mask_c, slots):
    """mmdyn_tconv_out3_bn_bce_rows_grad: with w = 1 dlogit and the published logits equal mmdyn_tconv_out3_bn_bce's bit for bit and
    the rows equal mmdyn_tconv_out3_bn_bce_rows's to the bound of that kernel's own test against the unfused pair (1e-7: fp64 atomics
    in another order); with random w every sample's block is the w = 1 block times w_b, bitwise; the rows stay unweighted."""
    B, S, n_slots, gs = G * Bg, 2 * H, 8, 0.29
    prec = {torch.float32: "fp32", torch.bfloat16: "bf16s", torch.float16: "fp16s"}[dtype]
    y = (rnd(B, 32, H, H, seed=60) * 2 + 0.3).to(dtype)
    mean, rstd = rnd(G, 32, seed=61) * 0.3, rnd(G, 32, seed=62).abs() + 0.5
    gamma, beta = rnd(32, seed=63) + 1.2, rnd(32, seed=64)
    Wt = rnd(32, 3, 4, 4, seed=65, scale=0.2)
    g = torch.Generator().manual_seed(66)
    target = torch.rand(Bg, 3, S, S, generator=g).to(DEV)
    mask = (torch.rand(Bg, mask_c, S, S, generator=g) > 0.3).float().to(DEV) if mask_c else None
    keep = 0
    prev = ops.B.precision
    ops.B.precision = prec
    try:
        args = (nhwc_rows(y).to(DEV), mean.to(DEV), rstd.to(DEV), gamma.to(DEV), beta.to(DEV), Wt.to(DEV))
        mk = dict(mask=mask, mask_channels=max(mask_c, 1))
        n = B * 3 * S * S
        # siblings
        out0, d0 = torch.empty(Bg, 3, S, S, device=DEV), torch.empty(n, device=DEV)
        HIP.tconv_out3_bn_bce(*args, out0, keep, target, d0, f64(n_slots), slots, gs, G, Bg, H, H,
                              unmasked_slots=f64(n_slots) if mask_c else None, **mk)
        rows0, rows0_u = f64(n_slots, Bg), f64(n_slots, Bg)
        HIP.tconv_out3_bn_bce_rows(*args, None, -1, target, rows0, slots, G, Bg, H, H, unmasked_rows=rows0_u if mask_c else None, **mk)
        # w = 1
        out1 = torch.empty(Bg, 3, S, S, device=DEV)
        buf, d1 = guarded(n)
        rows1, rows1_u = f64(n_slots, Bg), f64(n_slots, Bg)
        HIP.tconv_out3_bn_bce_rows_grad(*args, out1, keep, target, d1, torch.ones(Bg, device=DEV), rows1, slots, gs, G, Bg, H, H,
                                        unmasked_rows=rows1_u if mask_c else None, **mk)
        torch.cuda.synchronize()
        assert torch.equal(d1, d0) and torch.equal(out1, out0) and guards_intact(buf)
        print("fused rows+grad", G, Bg, H, dtype, "rows vs the rows launch", rel(rows1, rows0))
        assert rel(rows1, rows0) < 1e-7 and (not mask_c or rel(rows1_u, rows0_u) < 1e-7)
        for gi, sl in enumerate(slots):
            if sl < 0:
                assert float(d1.reshape(G, -1)[gi].abs().max()) == 0.0
        # random weights
        w = W.weights(Bg).to(DEV)
        buf, d2 = guarded(n)
        rows2 = f64(n_slots, Bg)
        HIP.tconv_out3_bn_bce_rows_grad(*args, None, -1, target, d2, w, rows2, slots, gs, G, Bg, H, H, **mk)
        torch.cuda.synchronize()
        assert torch.equal(d2, scaled_rows(d1, w, G, Bg)) and guards_intact(buf)
        assert rel(rows2, rows1) < 1e-7
        # fp64 ATen
        yd = y.double()
        xh = (yd.reshape(G, Bg, 32, H, H) - mean.double().reshape(G, 1, 32, 1, 1)) * rstd.double().reshape(G, 1, 32, 1, 1)
        u = (xh * gamma.double().reshape(1, 1, 32, 1, 1) + beta.double().reshape(1, 1, 32, 1, 1)).reshape(B, 32, H, H)
        lg = F.conv_transpose2d(u * torch.sigmoid(u), Wt.double(), stride=2, padding=1).reshape(G, Bg, 3, S, S)
        md = 1.0 if mask is None else mask.double().cpu()
        want = (md * (torch.sigmoid(lg * md) - target.double().cpu() * md) * gs) * w.double().cpu().reshape(1, Bg, 1, 1, 1)
        for gi, sl in enumerate(slots):
            if sl < 0:
                want[gi] = 0
        assert rel(d2.reshape(G, Bg, 3, S, S), want) < 2e-5
        # bad arguments
        with pytest.raises(ops._lib.MmdynError):
            HIP.tconv_out3_bn_bce_rows_grad(*args, None, -1, target, d2, w, rows2, [8] + list(slots[1:]), gs, G, Bg, H, H, **mk)
        with pytest.raises(ValueError):
            HIP.tconv_out3_bn_bce_rows_grad(*args, None, -1, target, d2, torch.ones(Bg + 1, device=DEV), rows2, slots, gs, G, Bg, H, H, **mk)
        with pytest.raises(ValueError):
            HIP.tconv_out3_bn_bce_rows_grad(*args, None, -1, target, None, w, rows2, slots, gs, G, Bg, H, H, **mk)
    finally:
        ops.B.precision = prev


# ---- the engine, the module API and the Problem API ---------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
@pytest.mark.parametrize("name", W.MVAE_NAMES)
def test_fixture_fused_engine(golden_dir, name, precision):
    TW.check_engine_fixture(golden_dir, DEV, name, precision)


@pytest.mark.parametrize("name", W.MVAE_NAMES)
def test_fixture_module_api(golden_dir, name):
    TW.check_module_fixture(golden_dir, DEV, name)


def test_fixture_vae_module_api(golden_dir):
    TW.check_vae_fixture(golden_dir, DEV)


@pytest.mark.parametrize("B,kl", [(5, "sample"), (5, "batch"), (37, "sample"), (37, "batch"), (130, "sample"), (130, "batch")])
def test_engine_vs_oracle_fp32_pose(B, kl):
    TW.check_engine_vs_oracle(DEV, True, B, kl, "fp32")


@pytest.mark.parametrize("B", [37, 130])
def test_engine_vs_oracle_fp32x3_nopose(B):
    """Without a pose decoder there are no ReLU knife edges: no tensor is left out."""
    TW.check_engine_vs_oracle(DEV, False, B, "sample", "fp32x3")


def _one_step(precision, B, w, kl, seed=11):
    inputs, targets = seeded_batch(B, 5)
    gi, gt = [x.to(DEV) for x in inputs], [x.to(DEV) for x in targets]
    m = T.build("cnn-mvae", True, True, DEV)
    step = MVAEStep(m, noise=NoiseSource(seed), precision=precision)
    loss = float(step.train_step(gi, gt, 0.02, sample_weight=w, kl=kl))
    flat = step.params.flat.clone()
    step.close()
    return loss, flat


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_ones_equals_unweighted_step(precision):
    """Parameters after one optimiser step with w = 1 (kl="sample") against the unweighted step on the same Philox noise.  Two
    unweighted eager steps are compared first: bitwise repeatable -> bitwise equality is demanded; otherwise four times the measured
    run-to-run difference (relative L2 over the flat parameter vector).  Measured: docs/LAB_NOTES.md M."""
    B = 37
    l0, p0 = _one_step(precision, B, None, "batch")
    l0b, p0b = _one_step(precision, B, None, "batch")
    l1, p1 = _one_step(precision, B, torch.ones(B, device=DEV), "sample")
    run_to_run = float((p0 - p0b).double().norm() / p0.double().norm())
    diff = float((p1 - p0).double().norm() / p0.double().norm())
    print(f"[{precision}] unweighted run-to-run {run_to_run:.3e} (bitwise: {torch.equal(p0, p0b)}); w = 1 against unweighted {diff:.3e} "
          f"(bitwise: {torch.equal(p1, p0)}); losses {l0!r} {l0b!r} {l1!r}")
    if torch.equal(p0, p0b):
        assert torch.equal(p1, p0)
    else:
        assert diff <= 4 * run_to_run
    assert l1 == pytest.approx(l0, rel=1e-6)


def test_graph_replay_with_weights():
    """Two replays with two weight vectors equal the two eager steps (the criterion of test_graph_replay_equals_eager_steps: losses
    to 1e-6 relative from the same state and Philox stream); an unweighted graphed step afterwards still matches its eager twin."""
    B, klw = 32, 0.02
    inputs, targets = seeded_batch(B, 5)
    gi, gt = [x.to(DEV) for x in inputs], [x.to(DEV) for x in targets]
    ws = [W.weights(B, 3).to(DEV).abs(), W.weights(B, 4).to(DEV).abs(), W.weights(B, 8).to(DEV).abs(), None]
    runs, rows = [], []
    for graphed in (False, True):
        m = T.build("cnn-mvae", True, True, DEV)
        step = MVAEStep(m, noise=NoiseSource(11))
        losses, rr = [], []
        for w in ws:
            fn = step.train_step_graphed if graphed else step.train_step
            losses.append(float(fn(gi, gt, klw, sample_weight=w, kl="sample")))
            if w is not None:
                rr.append(step.last_rows["rows"].clone())
        runs.append(losses)
        rows.append(rr)
        if graphed:
            assert step._graph is not None and ("weighted", "sample") not in step._graph[0]      # (re-captured for the unweighted step)
        step.close()
    print("eager", runs[0], "graphed", runs[1])
    assert runs[0] == pytest.approx(runs[1], rel=1e-6)
    for a, b in zip(*rows):
        assert torch.allclose(a, b, rtol=1e-5)
    assert len(set(runs[1])) == len(ws)


def test_eval_and_mask_and_unfused_fallback():
    """The weighted step with a loss mask, and with the BCE term out of the last layer's epilogue (the unfused twin kernels): the same
    loss and gradients as the fused launch, to fp32 summation order."""
    import mmdyn_hip.engine as E
    B = 5
    inputs, targets = seeded_batch(B, 1234, with_pose=False)
    eps, masks = seeded_noise(B, 256, 3, 4, 4321)
    mask, w = C.loss_mask(B, 1), W.weights(B)
    res = []
    for fused in (True, False):
        prev, E.FUSED_BCE = E.FUSED_BCE, fused
        try:
            res.append(TW.engine_grads(DEV, False, inputs, targets, eps, masks, 0.3, w, "sample", mask, "fp32"))
        finally:
            E.FUSED_BCE = prev
    assert res[1][1] == pytest.approx(res[0][1], rel=1e-6)
    for k in res[0][4]:
        assert TW.rel_l2(res[1][4][k], res[0][4][k]) < 1e-5, k
    for r in res:
        r[0].close()


@pytest.mark.parametrize("fused", [False, True])
def test_train_batch(fused):
    out = TW.check_train_batch(DEV, fused)
    np.testing.assert_allclose(out[True]["rows"].cpu().numpy(), out[False]["rows"].cpu().numpy(), rtol=1e-5)
