"""Eval-mode backward on a real MI355X: the layer schedules with BatchNorm frozen at its running estimates
(``training=False`` forward, then ``encoder_trunk_backward`` / ``decoder_backward``) against the CPU oracle under ``O.eval_mode()`` +
autograd, in both fp32-grade arithmetics; the module API (``eval_grad()``) against the reference's file tests/golden/eval_grad.npz;
and one cnn-vae at 128 pixels against the oracle.  Tolerances as in tests/test_layers_gpu.py beside it: forward 2e-5, gradients
1e-3 relative L2 per tensor."""
import pytest
import torch

import eval_grad_cases as C
import test_eval_grad_emu as TE
import test_model_emu as TM
from oracle import mvae_oracle as O
from mmdyn_hip import layers, ops
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.models import functional as Fn
from mmdyn_hip.models.shapes import state_dict_shapes
from mmdyn_hip.utils.seeded_init import seeded_running_stats, seeded_state_dict
from test_layers_gpu import rel, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(params=[True, False], ids=["fp32x3", "fp32"])
def arithmetic(request):
    prev, ops.B.fp32_split = ops.B.fp32_split, request.param
    yield request.param
    ops.B.fp32_split = prev


def state():
    return O.split_state(seeded_running_stats(seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=True), 0)))


_REF = {}


def oracle_once(key, fn):
    """The oracle's result of one (stack, B): computed once, shared by the two arithmetics, never modified."""
    if key not in _REF:
        _REF.clear()
        _REF[key] = fn()
    return _REF[key]


@pytest.mark.parametrize("B,G", [(4, 1), (6, 2), (32, 1)])
def test_encoder_trunk_eval_backward(B, G, arithmetic):
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    dh = torch.randn(B, 512, generator=torch.Generator().manual_seed(2))

    def oracle():
        prm, buf = state()
        xo = x.clone().requires_grad_(True)
        with O.eval_mode():
            h = O.image_encoder_trunk(xo, prm, "visual_encoder", buf)
        keys = ["visual_encoder." + k for k in layers.ENC_KEYS]
        gs = torch.autograd.grad((h * dh).sum(), [prm[k] for k in keys] + [xo])
        return prm, buf, h.detach(), dict(zip(layers.ENC_KEYS, gs[:-1])), gs[-1]

    prm, buf, h_ref, g_ref, dx_ref = oracle_once(("enc", B), oracle)
    P, Bf = sub(prm, "visual_encoder", DEV), sub(buf, "visual_encoder", DEV)
    before = {k: v.clone() for k, v in Bf.items()}
    h, ctx = layers.encoder_trunk_forward(P, Bf, x.to(DEV), G=G, training=False)
    assert rel(h, h_ref) < 2e-5
    grads = {k: torch.zeros_like(P[k]) for k in layers.ENC_KEYS}
    dx = layers.encoder_trunk_backward(P, ctx, dh.to(DEV), grads, need_dx=True)
    for k in Bf:
        assert torch.equal(Bf[k], before[k]), k
    d = rel(dx, dx_ref)
    print("dx rel L2", d)
    assert d < 1e-3
    for k in layers.ENC_KEYS:
        assert rel(grads[k], g_ref[k]) < 1e-3, k


@pytest.mark.parametrize("B,G", [(4, 1), (8, 4), (32, 2)])
def test_decoder_eval_backward(B, G, arithmetic):
    z = torch.randn(B, 256, generator=torch.Generator().manual_seed(3))
    dl = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(4))

    def oracle():
        prm, buf = state()
        zo = z.clone().requires_grad_(True)
        with O.eval_mode():
            out = O.image_decoder(zo, prm, "tactile_decoder", buf)
        keys = ["tactile_decoder." + k for k in layers.DEC_KEYS]
        gs = torch.autograd.grad((out * dl).sum(), [prm[k] for k in keys] + [zo])
        return prm, buf, out.detach(), dict(zip(layers.DEC_KEYS, gs[:-1])), gs[-1]

    prm, buf, ref, g_ref, dz_ref = oracle_once(("dec", B), oracle)
    P, Bf = sub(prm, "tactile_decoder", DEV), sub(buf, "tactile_decoder", DEV)
    before = {k: v.clone() for k, v in Bf.items()}
    out, ctx = layers.decoder_forward(P, Bf, z.to(DEV), G=G, training=False)
    assert rel(out, ref) < 2e-5
    grads = {k: torch.zeros_like(P[k]) for k in layers.DEC_KEYS}
    dz = layers.decoder_backward(P, ctx, dl.to(DEV), grads)
    for k in Bf:
        assert torch.equal(Bf[k], before[k]), k
    d = rel(dz, dz_ref)
    print("dz rel L2", d)
    assert d < 1e-3
    for k in layers.DEC_KEYS:
        assert rel(grads[k], g_ref[k]) < 1e-3, k
    # no parameter needed: dz alone, the same value
    out, ctx = layers.decoder_forward(P, Bf, z.to(DEV), G=G, training=False)
    dz0 = layers.decoder_backward(P, ctx, dl.to(DEV), {}, need=set())
    assert rel(dz0, dz_ref) < 1e-3


def test_module_eval_grad_golden_on_the_device(golden_dir):
    TE.check_module_golden(golden_dir, DEV)


def test_vae_128_eval_grad_against_the_oracle():
    """cnn-vae at 128 pixels, B = 4, in eval() with eval_grad(): loss, every parameter gradient and the image gradient against the
    oracle.  (The 128-pixel stack is this project's extension: the reference has no architecture of that size, so there is no
    reference file -- the oracle, pinned to the reference at 64 pixels, is the yardstick.)"""
    B, S = 4, 128
    g = torch.Generator().manual_seed(8)
    x = torch.rand(B, 3, S, S, generator=g)
    eps = torch.randn(B, 256, generator=g)
    sd = seeded_running_stats(seeded_state_dict(state_dict_shapes("cnn-vae", size=S), 0))
    prm, buf = O.split_state(sd)
    xo = x.clone().requires_grad_(True)
    with O.eval_mode():
        recon, mu, lv = O.vae_forward(prm, xo, eps, None, buf)
        loss_o = O.elbo_loss(recon, x, mu, lv, C.KL_WEIGHT)
    keys = list(prm)
    gs = torch.autograd.grad(loss_o, [prm[k] for k in keys] + [xo])
    m = TM.build("cnn-vae", False, None, "cpu", size=S)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    m = m.to(DEV).eval().eval_grad()
    m.noise = InjectedNoise([eps], [])
    xd = x.to(DEV).requires_grad_(True)
    recon, mu, lv = m(xd)
    loss = (Fn.BCEWithLogitsSumFn.apply(recon, x.to(DEV), None) + C.KL_WEIGHT * Fn.KLFn.apply(mu, lv)) / B
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(loss_o.detach()), rel=1e-4)
    named = dict(m.named_parameters())
    for k, gr in zip(keys, gs[:-1]):
        assert rel(named[k].grad, gr) < 1e-3, k
    d = rel(xd.grad, gs[-1])
    print("x.grad rel L2 at 128 px", d)
    assert d < 1e-3
