"""Eval-mode backward on the CPU: gradients through models whose BatchNorm is frozen at its running estimates (``model.eval()`` with
``eval_grad()``), and the input-image gradient of the encoder trunk (both modes), with the emulation backend of
tests/emu_backend_evalgrad.py.  Yardsticks: tests/golden/eval_grad.npz -- the reference's MVAE in ``eval()`` on the seeded case of
tests/eval_grad_cases.py: loss, every parameter gradient, both image gradients, the decoders' dz -- and the oracle under
``O.eval_mode()`` with torch autograd, itself pinned to that file here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cond_cases as CC
import eval_grad_cases as C
import test_model_emu as TM
from emu_backend_evalgrad import EmuBackendEvalGrad
from mmdyn_hip import layers, ops
from mmdyn_hip.models import InjectedNoise, setup_model
from mmdyn_hip.models import functional as Fn
from mmdyn_hip.models.shapes import state_dict_shapes
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise, seeded_running_stats, seeded_state_dict
from oracle import mvae_oracle as O
from test_oracle_golden import load, summarize

OREL = 1e-5        # oracle against the reference's file: both fp32 autograd on the CPU
GREL = 1e-3        # the project's gradient tolerance (tests/test_layers_gpu.py): relative L2 per tensor


@pytest.fixture(autouse=True)
def emu_evalgrad():
    old = ops.set_backend(EmuBackendEvalGrad())
    yield
    ops.set_backend(old)


def rel_l2(got, want):
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    return float((got - want).norm() / (want.norm() + 1e-30))


def golden_close(got, entry, tol, what):
    """A tensor against its entry of eval_grad.npz: stored whole (<= C.FULL elements) -> relative L2; stored as summarize(t, 256)
    -> the L2 norm, and the error of the 256 evenly spaced elements measured against the share of the tensor's norm that a subset of
    that size carries on average (an estimate of the relative L2 error from the sample)."""
    got = got.detach().cpu()
    if got.numel() <= C.FULL or tuple(np.shape(entry)) == tuple(got.shape):
        d = rel_l2(got, entry)
        print(what, "rel L2", d)
        assert d < tol, (what, d)
        return
    s = summarize(got, 256)
    want_n, n, k = float(entry[1]), float(entry[2]), len(entry) - 3
    assert n == got.numel(), what
    dn = abs(s[1] - want_n) / max(want_n, 1e-30)
    d = float(np.linalg.norm(s[3:] - entry[3:])) / max(want_n * (k / n) ** 0.5, 1e-30)
    print(what, "norm", dn, "sampled rel L2", d)
    assert dn < tol and d < tol, (what, dn, d)


def eval_state(name="cnn-mvae", **kw):
    return seeded_running_stats(seeded_state_dict(state_dict_shapes(name, **kw), 0))


def masked_poe(mus, lvs, masks):
    """vae.py:311-318 per row: expert m takes part in row b where masks[m][b] (the prior, first, always does)."""
    T = torch.stack([m[:, None] / ((torch.exp(lv) + O.POE_EPS) + O.POE_EPS) for lv, m in zip(lvs, masks)])
    mu = (torch.stack(mus) * T).sum(0) / T.sum(0)
    return mu, torch.log(1.0 / T.sum(0) + O.POE_EPS)


def oracle_joint(state, inputs, targets, eps, condition=None, available=None, dtype=torch.float32):
    """The joint pass in eval mode with autograd: (loss, {key: grad}, [d visual, d tactile], recons)."""
    prm, buf = O.split_state(state, dtype)
    v, t, p = (x.clone().to(dtype) for x in inputs)
    v.requires_grad_(True), t.requires_grad_(True)
    tg = [x.to(dtype) for x in targets]
    cond = None if condition is None else condition.to(dtype)
    with O.eval_mode():
        if available is None:
            vr, tr, pr, mu, lv = O.mvae_forward(prm, v, t, p, eps.to(dtype), iter([None, None]), True, buf, cond)
        else:
            B, L = v.shape[0], prm["visual_encoder.linear_means.bias"].shape[0]
            heads = [(torch.zeros(B, L, dtype=dtype), torch.zeros(B, L, dtype=dtype)),
                     O.image_encoder(v, prm, "visual_encoder", None, buf, cond), O.image_encoder(t, prm, "tactile_encoder", None, buf, cond),
                     O.pose_encoder(p, prm)]
            masks = [torch.ones(B, dtype=dtype)] + [available[:, i].to(dtype) for i in range(3)]
            mu, lv = masked_poe([h[0] for h in heads], [h[1] for h in heads], masks)
            z = O.reparametrize(mu, lv, eps.to(dtype))
            vr, tr = O.image_decoder(z, prm, "visual_decoder", buf, cond), O.image_decoder(z, prm, "tactile_decoder", buf, cond)
            pr = O.pose_decoder(z, prm)
        loss = O.mvae_elbo_loss([vr, tr, pr], tg, mu, lv, C.KL_WEIGHT, C.POSE_MULTIPLIER)
    keys = list(prm)
    gs = torch.autograd.grad(loss, [prm[k] for k in keys] + [v, t], allow_unused=True)
    return loss.detach(), dict(zip(keys, gs[:len(keys)])), list(gs[len(keys):]), (vr.detach(), tr.detach(), pr.detach())


def module_loss(recons, targets, mu, lv):
    """problems.py:421-458 (reduce=None) on the module API's loss Functions."""
    B = targets[0].shape[0]
    rec = Fn.BCEWithLogitsSumFn.apply(recons[0], targets[0], None) + Fn.BCEWithLogitsSumFn.apply(recons[1], targets[1], None) \
        + C.POSE_MULTIPLIER * Fn.MSESumFn.apply(recons[2], targets[2])
    return (rec + C.KL_WEIGHT * Fn.KLFn.apply(mu, lv)) / B


def eval_model(device, kw=None, state=None):
    m = setup_model("cnn-mvae", cross_modal=True, **(kw if kw is not None else dict(TM.MODEL_KW, use_pose=True)))
    sd = seeded_running_stats(seeded_state_dict(m.state_dict(), 0)) if state is None else state
    m.load_state_dict(sd)
    return m.to(device).eval()


def module_joint(m, device, inputs, targets, eps, condition=None, available=None):
    v, t, p = (x.clone().to(device) for x in inputs)
    v.requires_grad_(True), t.requires_grad_(True)
    m.noise = InjectedNoise([eps], [])
    kw = {} if available is None else {"available": available.to(device)}
    vr, tr, pr, mu, lv = m([v, t], pose=p, condition=None if condition is None else condition.to(device), **kw)
    loss = module_loss([vr, tr, pr], [x.to(device) for x in targets], mu, lv)
    m.zero_grad()
    loss.backward()
    return loss.detach(), {k: q.grad for k, q in m.named_parameters()}, [v.grad, t.grad], (vr.detach(), tr.detach(), pr.detach())


def test_oracle_eval_mode_autograd_reproduces_the_reference(golden_dir):
    g = load(golden_dir, "eval_grad.npz")
    inputs, targets, eps, z, r = C.case()
    assert np.array_equal(eps.numpy(), g["eps"]) and np.array_equal(z.numpy(), g["z"])
    loss, grads, gx, _ = oracle_joint(eval_state(use_pose=True), inputs, targets, eps)
    assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-6)
    for k, gr in grads.items():
        golden_close(gr, g["grad/" + k], OREL, k)
    for name, gr in zip(("visual", "tactile"), gx):
        golden_close(gr, g[f"gx/{name}"], OREL, "d " + name)
        golden_close(gr[0], g[f"gx/{name}0"], OREL, "d " + name + "[0]")
    prm, buf = O.split_state(eval_state(use_pose=True))
    for name in ("visual", "tactile"):
        zz = z.clone().requires_grad_(True)
        with O.eval_mode():
            (O.image_decoder(zz, prm, name + "_decoder", buf) * r).sum().backward()
        golden_close(zz.grad, g[f"dz/{name}"], OREL, "dz " + name)


def check_module_golden(golden_dir, device):
    """Module API with eval_grad() against the reference's file: loss, every parameter gradient, both image gradients, decoder dz;
    buffers bit-equal before and after; forward bit-equal to the same call without the flag."""
    g = load(golden_dir, "eval_grad.npz")
    inputs, targets, eps, z, r = C.case()
    m = eval_model(device)
    before = {k: b.clone() for k, b in m.named_buffers()}
    with torch.no_grad():
        m.noise = InjectedNoise([eps], [])
        plain = m([inputs[0].to(device), inputs[1].to(device)], pose=inputs[2].to(device))
    assert m.eval_grad() is m
    loss, grads, gx, recons = module_joint(m, device, inputs, targets, eps)
    for a, b in zip(recons, plain[:3]):
        assert torch.equal(a, b)                                   # the same launches: bit-identical forward
    print("loss", float(loss), "reference", float(g["loss"]))
    assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-4)
    for k, gr in grads.items():
        assert gr is not None, k
        golden_close(gr, g["grad/" + k], GREL, k)
    for name, gr in zip(("visual", "tactile"), gx):
        golden_close(gr, g[f"gx/{name}"], GREL, "d " + name)
        golden_close(gr[0], g[f"gx/{name}0"], GREL, "d " + name + "[0]")
    for name, dec in (("visual", m.visual_decoder), ("tactile", m.tactile_decoder)):
        zz = z.clone().to(device).requires_grad_(True)
        (dec(zz) * r.to(device)).sum().backward()
        golden_close(zz.grad, g[f"dz/{name}"], GREL, "dz " + name)
    for k, b in m.named_buffers():
        assert torch.equal(b, before[k]), k


def test_module_eval_grad_golden(golden_dir):
    check_module_golden(golden_dir, "cpu")


def test_eval_forward_is_graph_free_without_the_flag_and_under_no_grad():
    inputs, _, eps, z, _ = C.case()
    m = eval_model("cpu")
    x = inputs[0].clone().requires_grad_(True)
    zz = z.clone().requires_grad_(True)
    assert not m.visual_encoder.trunk(x).requires_grad and not m.visual_decoder(zz).requires_grad
    m.eval_grad()
    assert m.visual_encoder.trunk(x).requires_grad and m.visual_decoder(zz).requires_grad
    with torch.no_grad():
        assert not m.visual_encoder.trunk(x).requires_grad and not m.visual_decoder(zz).requires_grad
    m.eval_grad(False)
    assert not m.visual_encoder.trunk(x).requires_grad and not m.visual_decoder(zz).requires_grad
    # callable on a bare Encoder / Decoder
    assert m.visual_decoder.eval_grad() is m.visual_decoder and m.visual_decoder(zz).requires_grad
    assert not m.tactile_decoder(zz).requires_grad


def test_sixteen_bit_storage_with_the_flag_raises():
    _, _, _, z, _ = C.case()
    m = eval_model("cpu").eval_grad()
    prev, layers.ACT_DTYPE = layers.ACT_DTYPE, torch.bfloat16
    try:
        with pytest.raises(NotImplementedError, match="fp32 only"):
            m.visual_decoder(z.clone().requires_grad_(True))
    finally:
        layers.ACT_DTYPE = prev


class CountingBackend:
    """Forwards every op to ``inner`` and counts the calls by name."""

    def __init__(self, inner):
        self.inner, self.count = inner, {}

    def __getattr__(self, name):
        attr = getattr(self.inner, name)
        if not callable(attr):
            return attr

        def call(*a, **k):
            self.count[name] = self.count.get(name, 0) + 1
            return attr(*a, **k)
        return call


def test_frozen_decoder_gives_dz_without_parameter_gradient_launches(golden_dir):
    g = load(golden_dir, "eval_grad.npz")
    _, _, _, z, r = C.case()
    dec = eval_model("cpu").eval_grad().visual_decoder
    for q in dec.parameters():
        q.requires_grad_(False)
    zz = z.clone().requires_grad_(True)
    counting = CountingBackend(ops.B)
    old = ops.set_backend(counting)
    try:
        (dec(zz) * r).sum().backward()
    finally:
        ops.set_backend(old)
    golden_close(zz.grad, g["dz/visual"], GREL, "dz visual (frozen decoder)")
    assert all(q.grad is None for q in dec.parameters())
    for name in ("wgrad_tn", "wgrad_out3_bn", "wgrad_reduce", "colsum", "bn_bwd_finalize", "bn_swish_bwd_reduce", "bn_swish_bwd_apply"):
        assert counting.count.get(name, 0) == 0, (name, counting.count)
    assert counting.count["bn_eval_swish_bwd"] == 3 and counting.count["igemm_nt_dgrad_bn"] == 3


def test_one_trainable_parameter_gets_exactly_its_gradient(golden_dir):
    g = load(golden_dir, "eval_grad.npz")
    _, _, _, z, r = C.case()
    dec = eval_model("cpu").eval_grad().visual_decoder
    for k, q in dec.named_parameters():
        q.requires_grad_(k == "hallucinate.0.weight")
    counting = CountingBackend(ops.B)
    old = ops.set_backend(counting)
    try:
        (dec(z.clone()) * r).sum().backward()
    finally:
        ops.set_backend(old)
    for k, q in dec.named_parameters():
        assert (q.grad is not None) == (k == "hallucinate.0.weight"), k
    assert counting.count["wgrad_tn"] == 1 and counting.count.get("colsum", 0) == 0 and counting.count.get("bn_bwd_finalize", 0) == 0
    # d(sum logits * r) / d hallucinate.0.weight against the oracle (the file holds the ELBO's gradients, not this functional's)
    prm, buf = O.split_state(eval_state(use_pose=True))
    with O.eval_mode():
        (O.image_decoder(z, prm, "visual_decoder", buf) * r).sum().backward()
    d = rel_l2(dec.hallucinate[0].weight.grad, prm["visual_decoder.hallucinate.0.weight"].grad)
    print("hallucinate.0.weight rel L2", d)
    assert d < GREL


def test_train_mode_image_gradient():
    """ImageEncoderTrunkFn returns dL/dx in train mode too: x.grad against the oracle's (batch-statistics BatchNorm, dropout mask)."""
    B = 4
    inputs, _ = seeded_batch(B, 1234, with_pose=False)
    eps, masks = seeded_noise(B, 256, 1, 1, 4321)
    sd = seeded_state_dict(state_dict_shapes("cnn-vae"), 0)
    prm, buf = O.split_state(sd)
    xo = inputs[0].clone().requires_grad_(True)
    recon, mu, lv = O.vae_forward(prm, xo, eps[0], masks[0], buf)
    O.elbo_loss(recon, inputs[0], mu, lv, C.KL_WEIGHT).backward()
    m = TM.build("cnn-vae", False, None, "cpu")
    m.noise = InjectedNoise(eps, masks)
    x = inputs[0].clone().requires_grad_(True)
    recon, mu, lv = m(x)
    loss = (Fn.BCEWithLogitsSumFn.apply(recon, inputs[0], None) + C.KL_WEIGHT * Fn.KLFn.apply(mu, lv)) / B
    loss.backward()
    assert x.grad is not None
    d = rel_l2(x.grad, xo.grad)
    print("train-mode x.grad rel L2", d)
    assert d < GREL
    d = rel_l2(m.encoder.conv_net[0].weight.grad, prm["encoder.conv_net.0.weight"].grad)
    assert d < GREL


def compare_with_oracle(state, kw, inputs, targets, eps, condition=None, oracle_condition=None, available=None):
    lo, go, gxo, _ = oracle_joint(state, inputs, targets, eps, oracle_condition, available)
    m = eval_model("cpu", kw, {k: v.clone() for k, v in state.items()}).eval_grad()
    lm, gm, gxm, _ = module_joint(m, "cpu", inputs, targets, eps, condition, available)
    assert float(lm) == pytest.approx(float(lo), rel=1e-4)
    for k in go:
        if go[k] is None or float(go[k].norm()) == 0.0:            # (an expert absent in every row)
            assert gm[k] is None or float(gm[k].norm()) == 0.0, k
            continue
        d = rel_l2(gm[k], go[k])
        assert d < GREL, (k, d)
    for a, b in zip(gxm, gxo):
        d = rel_l2(a, b)
        print("image gradient rel L2", d)
        assert d < GREL


def test_eval_grad_with_an_availability_table():
    inputs, targets, eps, _, _ = C.case()
    available = torch.tensor([[1, 1, 1], [1, 0, 0], [0, 1, 1]], dtype=torch.float64)
    compare_with_oracle(eval_state(use_pose=True), dict(TM.MODEL_KW, use_pose=True), inputs, targets, eps, available=available)


def test_eval_grad_with_a_categorical_condition():
    inputs, targets, _, _, _ = C.case()
    eps = torch.randn(C.B, CC.LATENT, generator=torch.Generator().manual_seed(5))
    kw = CC.model_kw(True, True)
    idx = CC.indices(C.B, 22)
    m = setup_model("cnn-mvae", cross_modal=True, **kw)
    state = seeded_running_stats(seeded_state_dict(m.state_dict(), 0))
    compare_with_oracle(state, kw, inputs, targets, eps, condition=idx, oracle_condition=F.one_hot(idx, CC.CAT_DIM).float())


def test_emulated_kernel_plane_destination_and_partial_layout():
    """The emulation's own contract: the three planes sum to the fp32 destination bit for bit; the partial table has the layout of
    bn_swish_bwd_reduce (bn_bwd_finalize gives the same dgamma / dbeta from either); y may be None with da_is_du and no partial."""
    G, rpg, Cc = 2, 75, 32
    gen = torch.Generator().manual_seed(3)
    da, y = torch.randn(G * rpg, Cc, generator=gen), torch.randn(G * rpg, Cc, generator=gen)
    mean, rstd = 0.1 * torch.randn(G, Cc, generator=gen), 0.5 + torch.rand(G, Cc, generator=gen)
    gamma, beta = torch.randn(Cc, generator=gen), torch.randn(Cc, generator=gen)
    T = ops.B.colstats_tiles(rpg)
    dy, pl, partial = torch.empty_like(da), ops.Planes(G * rpg, Cc, da.device), torch.empty(G, T, 2, Cc)
    ops.B.bn_eval_swish_bwd(da, y, mean, rstd, gamma, beta, dy, partial, G, rpg, Cc, False, planes=pl)
    assert torch.equal(pl.float(), dy)
    ref = torch.empty(G, T, 2, Cc)
    ops.B.bn_swish_bwd_reduce(da, y, mean, rstd, gamma, beta, ref, G, rpg, Cc)
    out = []
    for p in (partial, ref):
        sums, dg, db = torch.empty(G, 2, Cc), torch.empty(Cc), torch.empty(Cc)
        ops.B.bn_bwd_finalize(p, sums, dg, db, None, G, T, Cc, 0.0)
        out.append((dg, db))
    assert rel_l2(out[0][0], out[1][0]) < 1e-6 and rel_l2(out[0][1], out[1][1]) < 1e-6
    a, b = torch.empty_like(da), torch.empty_like(da)
    ops.B.bn_eval_swish_bwd(da, None, mean, rstd, gamma, beta, a, None, G, rpg, Cc, True)
    ops.B.bn_eval_swish_bwd(da, y, mean, rstd, gamma, beta, b, None, G, rpg, Cc, True)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.B.bn_eval_swish_bwd(da, None, mean, rstd, gamma, beta, a, None, G, rpg, Cc, False)


def test_argument_errors_are_reported_without_a_gpu():
    """mmdyn_bn_eval_swish_bwd rejects null pointers and bad shapes on the host, before any launch (negative codes)."""
    from mmdyn_hip import _lib
    lib = _lib.load()
    q = 4096                                                         # any non-null address: nothing is dereferenced on these paths
    call = lambda da, y, dy, dyp, part, G, rpg, Cc, is_du: lib.mmdyn_bn_eval_swish_bwd(da, y, q, q, q, q, dy, dyp, part, G, rpg, Cc,
                                                                                         is_du, None)
    assert call(q, q, None, None, None, 1, 64, 32, 0) < 0            # no destination
    assert call(None, q, q, None, None, 1, 64, 32, 0) < 0            # no da
    assert call(q, None, q, None, None, 1, 64, 32, 0) < 0            # swish'(u) needs y
    assert call(q, None, None, q, q, 1, 64, 32, 1) < 0               # the tile sums need xhat, so y
    assert lib.mmdyn_bn_eval_swish_bwd(q, q, None, q, q, q, q, None, None, 1, 64, 32, 0, None) < 0
    for G, rpg, Cc in ((0, 64, 32), (1, 0, 32), (1, 64, 16), (1, 64, 48), (1, 64, 96), (1, 64, 512)):
        assert call(q, q, q, None, None, G, rpg, Cc, 0) < 0, (G, rpg, Cc)
