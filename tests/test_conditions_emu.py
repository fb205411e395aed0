"""Conditions end to end on the CPU: categorical (class-index) and real-valued conditions through the module API, the fused engine,
the serving engine and the problem layer, on the emulation backend (tests/emu_backend_cond.py), against tests/golden/conditions.npz
-- the reference's own results on the seeded cases of tests/cond_cases.py.  The ``check_*`` functions take the device: the GPU suite
(tests/test_conditions_gpu.py) runs the same checks on the HIP library."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cond_cases as C
import test_model_emu as TM
from emu_backend_cond import EmuBackendCond
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep, MVAEInference
from mmdyn_hip.models import setup_model, InjectedNoise
from mmdyn_hip.models.vae import Decoder, Encoder
from mmdyn_hip.problems.problems import Reconstruction, SeqModeling
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats
from test_oracle_golden import summarize, close_summary, close_params, load

# the tolerances tests/test_model_emu.py applies to mvae_conditional_B2.npz (loss / partials, outputs, gradient and parameter
# summaries) and to the serving engine's outputs (check_inference_engine)
REL, OUT_TOL, GRAD_TOL, SUM_TOL = 1e-4, dict(rtol=1e-4, atol=3e-5), 1e-3, 3e-5


@pytest.fixture(autouse=True)
def emu_cond():
    old = ops.set_backend(EmuBackendCond())
    yield
    ops.set_backend(old)


def build(name, categorical, use_pose=None, device="cpu", cross=True, running=False):
    m = setup_model(name, cross_modal=cross, **C.model_kw(categorical, use_pose))
    sd = seeded_state_dict(m.state_dict(), 0)
    m.load_state_dict(seeded_running_stats(sd) if running else sd)
    return m.to(device)


def dv(ts, device):
    return [t.to(device) for t in ts]


def problem_of(m, model_name, cls=SeqModeling):
    prob = cls.__new__(cls)
    prob._model, prob._kl_weight, prob._pose_multiplier, prob._conditional = m, C.KL_WEIGHT, C.POSE_MULTIPLIER, True
    prob._step = None
    prob.parameters = {"use_pose": True, "model_name": model_name, "mask_loss": False, "input_type": "visuotactile"}
    return prob


def check_grads(m, g, tag):
    for k, p_ in m.named_parameters():
        close_summary(summarize(p_.grad.cpu()), g[f"{tag}/grad/" + k], GRAD_TOL, "grad " + k)


def check_cond_columns(m, g):
    """The condition columns of the six conditional weight matrices, named explicitly: their gradient comes from the joined
    operand (no gradient flows to the condition itself)."""
    for k in C.COND_WEIGHTS:
        grad = dict(m.named_parameters())[k].grad
        assert grad.shape[1] in (512 + C.CAT_DIM, C.LATENT + C.CAT_DIM)
        cols = grad[:, -C.CAT_DIM:]
        assert float(cols.abs().max()) > 0
        close_summary(summarize(cols.cpu(), 256), g["a/grad_cond/" + k], GRAD_TOL, "condition columns of " + k)


def check_module_train(golden_dir, device):
    """(a) through the module API: the reference's seven model calls with class-index conditions, autograd, one Adam step."""
    from mmdyn_hip.problems.problems import FusedAdam
    g = load(golden_dir, "conditions.npz")
    m = build("cnn-mvae", True, True, device).train()
    assert m.visual_encoder.linear_means.weight.shape == (C.LATENT, 512 + C.CAT_DIM)
    assert m.visual_decoder.upsample[0].weight.shape == (6400, C.LATENT + C.CAT_DIM)
    assert m.pose_encoder.linear_means.weight.shape == (C.LATENT, 512)          # the pose MLPs stay unconditional
    inputs, targets, eps, masks, idx = C.train_case()
    prob = problem_of(m, "cnn-mvae")
    m.noise = InjectedNoise(eps, masks)
    partials, inner = [], prob._mvae_elbo_loss
    prob._mvae_elbo_loss = lambda *a, **k: (partials.append(inner(*a, **k)), partials[-1])[1]
    opt = FusedAdam(m.parameters(), lr=C.LR)
    opt.zero_grad()
    outputs, loss = prob._evaluate_mvae(x=dv(inputs, device), targets=dv(targets, device), condition=idx.to(device))
    loss.backward()
    print("loss", float(loss.detach()), "reference", float(g["a/loss"]))
    assert float(loss.detach()) == pytest.approx(float(g["a/loss"]), rel=REL)
    np.testing.assert_allclose([float(p.detach()) for p in partials], g["a/loss_partials"], rtol=REL)
    np.testing.assert_allclose(outputs["means"].detach().cpu().numpy(), g["a/means"], **OUT_TOL)
    np.testing.assert_allclose(outputs["recon_x"][2].detach().cpu().numpy(), g["a/recon2"], **OUT_TOL)
    check_grads(m, g, "a")
    check_cond_columns(m, g)
    opt.step()
    for k, p_ in m.named_parameters():
        close_params(summarize(p_.detach().cpu()), g["a/param_step0/" + k], GRAD_TOL, 1, "param " + k)


def check_engine_train(golden_dir, device, precision=None):
    """(a) through MVAEStep (eager): loss, the 7 partials, means, every gradient, the parameters after the Adam step."""
    g = load(golden_dir, "conditions.npz")
    m = build("cnn-mvae", True, True, device).train()
    inputs, targets, eps, masks, idx = C.train_case()
    inputs, targets = dv(inputs, device), dv(targets, device)
    kw = {} if precision is None else {"precision": precision}
    step = MVAEStep(m, lr=C.LR, pose_multiplier=C.POSE_MULTIPLIER, noise=InjectedNoise(eps, masks), **kw)
    assert step.categorical
    for cond in (idx, idx.unsqueeze(1).to(torch.int32)):                     # [B] int64 and [B,1] int32 are the same condition
        step.noise = InjectedNoise(eps, masks)
        loss = step.forward(inputs, targets, C.KL_WEIGHT, train=True, condition=cond.to(device))
        print(step.precision, "loss", float(loss), "reference", float(g["a/loss"]), "partials", step.partials[:7].cpu().numpy())
        assert float(loss) == pytest.approx(float(g["a/loss"]), rel=REL)
        np.testing.assert_allclose(step.partials[:7].cpu().numpy(), g["a/loss_partials"], rtol=REL)
        np.testing.assert_allclose(step.last["means"].cpu().numpy(), g["a/means"], **OUT_TOL)
        np.testing.assert_allclose(step.last["recon_x"][2].cpu().numpy(), g["a/recon2"], **OUT_TOL)
        handles = step.backward()
    check_grads(m, g, "a")
    check_cond_columns(m, g)
    step.optimizer_step(handles)
    for k, p_ in m.named_parameters():
        close_params(summarize(p_.detach().cpu()), g["a/param_step0/" + k], GRAD_TOL, 1, "param " + k)
    assert not step.bad_condition()
    step.check_condition()
    # interface: a condition is required; a float tensor is no class index; an index >= condition_dim is reported, not a fault
    with pytest.raises(ValueError):
        step.forward(inputs, targets, 1.0)
    with pytest.raises(ValueError, match="float32"):
        step.forward(inputs, targets, 1.0, condition=idx.to(device).float())
    bad = idx.clone()
    bad[1] = C.CAT_DIM
    step.noise = InjectedNoise(eps, masks)
    step.eval_step(inputs, targets, C.KL_WEIGHT, condition=bad.to(device))
    assert step.bad_condition()
    with pytest.raises(ValueError):
        step.check_condition()
    step.noise = InjectedNoise(eps, masks)
    step.eval_step(inputs, targets, C.KL_WEIGHT, condition=idx.to(device))
    assert not step.bad_condition()
    step.close()


def check_engine_rows(golden_dir, device, precision=None):
    """(e): score_step with class-index conditions against the reference's reduce=False rows of (a)."""
    g = load(golden_dir, "conditions.npz")
    m = build("cnn-mvae", True, True, device).train()
    inputs, targets, eps, masks, idx = C.train_case()
    kw = {} if precision is None else {"precision": precision}
    step = MVAEStep(m, pose_multiplier=C.POSE_MULTIPLIER, noise=InjectedNoise(eps, masks), **kw)
    res = step.score_step(dv(inputs, device), dv(targets, device), C.KL_WEIGHT, condition=idx.to(device), kl="batch")
    print("rows", res["rows"].cpu().numpy(), "reference", g["e/rows"])
    np.testing.assert_allclose(res["rows"].cpu().numpy(), g["e/rows"], rtol=REL)
    np.testing.assert_allclose(res["partials"].cpu().numpy(), g["e/pass_rows"], rtol=REL)
    step.close()


def check_onehot_equivalence(device):
    """A categorical model fed indices c and a real-valued conditional model with the same state_dict fed one_hot(c).float():
    bit-identical forward outputs and gradients (the join only copies)."""
    inputs, targets, eps, masks, idx = C.train_case()
    outs = []
    for categorical in (True, False):
        kw = dict(C.model_kw(True, True), categorical_conditions=categorical)
        m = setup_model("cnn-mvae", cross_modal=True, **kw)
        m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
        m.to(device).train()
        m.noise = InjectedNoise(eps[:1], masks[:2])
        cond = idx.to(device) if categorical else F.one_hot(idx, C.CAT_DIM).float().to(device)
        v, t, p, mu, lv = m(dv(inputs[:2], device), pose=inputs[2].to(device), condition=cond)
        (v.sum() + 2 * t.sum() + p.sum() + (mu * lv).sum()).backward()
        outs.append(([v, t, p, mu, lv], {k: p_.grad for k, p_ in m.named_parameters()}))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert torch.equal(a, b)
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


def serving(categorical, device, **kw):
    m = build("cnn-mvae", categorical, True, device, running=True).eval()
    return m, MVAEInference(m, **kw)


def check_inference_engine(golden_dir, device, categorical, precision="fp32x3"):
    """(b) / (c): MVAEInference.forward of the joint, visual-only and pose-only subsets and inference(n, c), noise injected, and
    the eval-mode module forward beside it."""
    g = load(golden_dir, "conditions.npz")
    tag = "b" if categorical else "c"
    inputs, eps, cond, z, cs = C.eval_case(categorical)
    inputs, cond, cs = dv(inputs, device), cond.to(device), cs.to(device)
    m, eng = serving(categorical, device, precision=precision)
    eng.use_graph = False                                   # injected noise: compare with the reference's vectors
    for who in ("engine", "module"):
        for name, (a, b, c) in C.SUBSETS.items():
            x, pose = [inputs[0] if a else None, inputs[1] if b else None], inputs[2] if c else None
            if who == "engine":
                eng.noise = InjectedNoise([eps[name].clone()], [])
                v, t, p, mu, lv = eng.forward(x, pose=pose, condition=cond)
            else:
                m.noise = InjectedNoise([eps[name].clone()], [])
                with torch.no_grad():
                    v, t, p, mu, lv = m(x, pose=pose, condition=cond)
            close_summary(summarize(v.cpu(), 256), g[f"{tag}/{name}/visual"], SUM_TOL, f"{who} {name} visual")
            close_summary(summarize(t.cpu(), 256), g[f"{tag}/{name}/tactile"], SUM_TOL, f"{who} {name} tactile")
            np.testing.assert_allclose(p.cpu().numpy(), g[f"{tag}/{name}/pose"], **OUT_TOL)
            np.testing.assert_allclose(mu.cpu().numpy(), g[f"{tag}/{name}/means"], **OUT_TOL)
            np.testing.assert_allclose(lv.cpu().numpy(), g[f"{tag}/{name}/log_var"], **OUT_TOL)
        if who == "engine":
            eng.noise = InjectedNoise([z.clone()], [])
            v, t = eng.inference(C.SAMPLE_N, cs)
        else:
            m.noise = InjectedNoise([z.clone()], [])
            with torch.no_grad():
                v, t = m.inference(C.SAMPLE_N, cs)
        close_summary(summarize(v.cpu(), 256), g[f"{tag}/inference/visual"], SUM_TOL, who + " inference visual")
        close_summary(summarize(t.cpu(), 256), g[f"{tag}/inference/tactile"], SUM_TOL, who + " inference tactile")
    assert not eng.bad_condition()
    return m, eng, inputs, cond


def check_vae(golden_dir, device):
    """(d): the categorical cnn-vae through Reconstruction._evaluate_model (the labels are the conditions) and inference."""
    g = load(golden_dir, "conditions.npz")
    x, labels, eps, masks, z, cs = C.vae_case()
    m = build("cnn-vae", True, None, device, cross=False).train()
    prob = problem_of(m, "cnn-vae", Reconstruction)
    prob._criterion = prob._elbo_loss
    m.noise = InjectedNoise(eps, masks)
    outputs, loss = prob._evaluate_model(x.to(device), labels.to(device))
    loss.backward()
    print("vae loss", float(loss.detach()), "reference", float(g["d/loss"]))
    assert float(loss.detach()) == pytest.approx(float(g["d/loss"]), rel=REL)
    np.testing.assert_allclose(outputs["means"].detach().cpu().numpy(), g["d/means"], **OUT_TOL)
    np.testing.assert_allclose(outputs["log_var"].detach().cpu().numpy(), g["d/log_var"], **OUT_TOL)
    close_summary(summarize(outputs["recon_x"].detach().cpu(), 256), g["d/recon"], SUM_TOL, "recon")
    check_grads(m, g, "d")
    m.eval()
    m.noise = InjectedNoise([z], [])
    with torch.no_grad():
        v = m.inference(C.SAMPLE_N, cs.to(device))
    close_summary(summarize(v.cpu(), 256), g["d/inference"], SUM_TOL, "inference")


# ---- the CPU suite ----------------------------------------------------------------------------------------------------------
def test_module_train(golden_dir):
    check_module_train(golden_dir, "cpu")


def test_engine_train(golden_dir):
    check_engine_train(golden_dir, "cpu")


def test_engine_rows(golden_dir):
    check_engine_rows(golden_dir, "cpu")


def test_onehot_equivalence():
    check_onehot_equivalence("cpu")


@pytest.mark.parametrize("categorical", [True, False], ids=["categorical", "real"])
def test_inference_engine(golden_dir, categorical):
    check_inference_engine(golden_dir, "cpu", categorical)


def test_categorical_vae(golden_dir):
    check_vae(golden_dir, "cpu")


class _Counting:
    """Wraps the active backend and counts the calls of the named ops."""

    def __init__(self, inner, names):
        self._inner, self.calls = inner, {n: 0 for n in names}

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if name in self.calls:
            def counted(*a, **k):
                self.calls[name] += 1
                return attr(*a, **k)
            return counted
        return attr


@pytest.mark.parametrize("categorical", [True, False], ids=["categorical", "real"])
def test_join_launch_count(categorical):
    """A conditional MVAEInference.forward of the joint subset: exactly 4 concat_condition calls (two heads, two decoders) and no
    repack2d_ld call for the join."""
    inputs, eps, cond, z, cs = C.eval_case(categorical)
    m, eng = serving(categorical, "cpu")
    counting = _Counting(ops.B, ["concat_condition", "repack2d_ld"])
    old = ops.set_backend(counting)
    try:
        eng.forward([inputs[0], inputs[1]], pose=inputs[2], condition=cond)
    finally:
        ops.set_backend(old)
    assert counting.calls == {"concat_condition": 4, "repack2d_ld": 0}


def test_three_call_form_kept():
    """A backend without concat_condition (the existing emulation) still gets the zero fill + two block copies."""
    from emu_backend_rows import EmuBackendRows
    from mmdyn_hip import layers
    old = ops.set_backend(_Counting(EmuBackendRows(), ["repack2d_ld"]))
    try:
        x, c = torch.rand(3, 64), torch.rand(3, 3)
        out = layers.concat_condition(x, c, 96)
        assert ops.B.calls["repack2d_ld"] == 2
        assert torch.equal(out, torch.cat((x, c, torch.zeros(3, 29)), -1))
        with pytest.raises(RuntimeError):
            layers.concat_condition(x, torch.tensor([0, 1, 2]), 96, 3)
    finally:
        ops.set_backend(old)


def test_interface_errors():
    inputs, eps, cond, z, cs = C.eval_case(True)
    m, eng = serving(True, "cpu")
    x = [inputs[0], inputs[1]]
    with pytest.raises(ValueError):
        eng.forward(x, pose=inputs[2])                                          # missing
    with pytest.raises(ValueError):
        eng.inference(2)
    with pytest.raises(ValueError, match="float32"):
        eng.forward(x, pose=inputs[2], condition=cond.float())                  # float condition for a categorical model
    with pytest.raises(ValueError):
        eng.forward(x, pose=inputs[2], condition=cond[:2])                      # wrong batch
    with pytest.raises(ValueError, match="float32"):
        m(x, pose=inputs[2], condition=cond.float())
    with pytest.raises(ValueError):
        m(x, pose=inputs[2])
    # an index >= condition_dim raises in the eager model paths (the reference asserts), each of them
    bad = cond.clone()
    bad[0] = C.CAT_DIM
    m.noise = None
    with torch.no_grad():
        with pytest.raises(ValueError, match="condition_dim"):
            m(x, pose=inputs[2], condition=bad)
        with pytest.raises(ValueError, match="condition_dim"):
            m.inference(3, bad)
        with pytest.raises(ValueError, match="condition_dim"):
            m.visual_encoder.heads(torch.rand(3, 512), bad)
        with pytest.raises(ValueError, match="condition_dim"):
            m.visual_decoder(torch.rand(3, C.LATENT), bad)
        m(x, pose=inputs[2], condition=cond)                                    # ... and a good call afterwards passes
    # the serving engine reports instead of raising, and is clear after a good request
    eng.forward(x, pose=inputs[2], condition=bad)
    assert eng.bad_condition()
    eng.forward(x, pose=inputs[2], condition=cond)
    assert not eng.bad_condition()
    # surplus condition: unconditional model
    plain = TM.build("cnn-mvae", True, True).eval()
    with pytest.raises(ValueError):
        MVAEInference(plain).forward([torch.rand(1, 3, 64, 64), None], condition=torch.zeros(1, 3))
    # the conditional mlp Encoder stays refused, with its reason; the mlp Decoder joins through the same kernel
    with pytest.raises(NotImplementedError, match="reference"):
        Encoder(input_dim=784, architecture="mlp", conditional=True, categorical_conditions=True, condition_dim=5)
    dec = Decoder(output_dim=20, layer_sizes=[32], latent_size=8, architecture="mlp", conditional=True,
                  categorical_conditions=True, condition_dim=5)
    zz, ii = torch.rand(4, 8, requires_grad=True), torch.tensor([4, 0, 2, 2])
    y = dec(zz, ii)
    lin = [mod for mod in dec.deconv_net if hasattr(mod, "weight")]
    want = F.linear(F.relu(F.linear(torch.cat((zz, F.one_hot(ii, 5).float()), -1), lin[0].weight, lin[0].bias)), lin[1].weight, lin[1].bias)
    np.testing.assert_allclose(y.detach().numpy(), want.detach().numpy(), rtol=1e-5, atol=1e-6)
    y.sum().backward()
    np.testing.assert_allclose(zz.grad.numpy(), torch.autograd.grad(want.sum(), zz)[0].numpy(), rtol=1e-5, atol=1e-6)


class _Labelled:
    """Stand-in dataset carrying class labels, and a loader over it."""
    targets = [0, 3, 1, 6, 2, 6]

    def __len__(self):
        return len(self.targets)


class _Loader(list):
    dataset = _Labelled()


def test_problem_layer(tmp_path):
    """Reconstruction on a labelled dataset builds a categorical model with condition_dim = max(targets) + 1; _sample returns
    images for it; an unlabelled dataset keeps the unconditional values."""
    ns = TM.args(problem_type="reconstruction", model_name="cnn-vae", input_type="visual", conditional=True, no_cuda=True,
                 latent_size=C.LATENT)
    loader = _Loader([(torch.rand(2, 3, 64, 64), torch.tensor([0, 6]))])
    prob = Reconstruction(ns, log_dir=str(tmp_path), train_loader=loader, test_loader=loader)
    assert prob._categorical_conditions and prob.condition_dim == 7
    m = prob.model
    assert m.categorical_conditions and m.encoder.linear_means.weight.shape == (C.LATENT, 512 + 7)
    assert m.decoder.upsample[0].weight.shape == (6400, C.LATENT + 7)
    imgs = prob._sample(n=5)
    assert tuple(imgs.shape) == (5, 3, 64, 64) and torch.isfinite(imgs).all()
    outputs, loss = prob._evaluate_model(*prob.parse_input(*loader[0]))
    assert torch.isfinite(loss) and tuple(outputs["recon_x"].shape) == (2, 3, 64, 64)
    plain = Reconstruction(TM.args(problem_type="reconstruction", model_name="cnn-vae", input_type="visual", no_cuda=True,
                                   latent_size=C.LATENT), log_dir=str(tmp_path), train_loader=loader, test_loader=loader)
    assert not plain._categorical_conditions and plain.condition_dim == 0
