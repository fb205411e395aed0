"""Per-sample weights in training on the CPU: L = (1/B) sum_b w_b * row_b and its gradients through the fused engine
(``MVAEStep(sample_weight=, kl=)``) and through the module API (the differentiable ``reduce=False`` rows), with the emulation backend
of tests/emu_backend_weighted.py.  Yardsticks: tests/golden/weighted_elbo.npz -- the reference's ``(w * rows).sum() / B`` and its
parameter gradients on the seeded cases of tests/rows_cases.py with the weights of tests/weighted_cases.py -- and, for the KL mode
the reference does not have, a torch-autograd restatement built on oracle.mvae_oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rows_cases as C
import test_elbo_rows_emu as TR
import test_model_emu as TM
import weighted_cases as W
from emu_backend_weighted import EmuBackendWeighted
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.models.shapes import state_dict_shapes
from mmdyn_hip.models.vae import NoiseSource
from mmdyn_hip.problems.problems import SeqModeling
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise, seeded_state_dict
from oracle import mvae_oracle as O
from test_oracle_golden import load

# tests/test_model_emu.py / test_fused_engine_vs_oracle: loss and partials 1e-4 relative, every gradient tensor 1e-3 relative L2
REL, GREL = 1e-4, 1e-3


@pytest.fixture(autouse=True)
def emu_weighted():
    old = ops.set_backend(EmuBackendWeighted())
    yield
    ops.set_backend(old)


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / (want.double().norm() + 1e-30))


def check_fixture_grads(g, name, named_grads):
    """Every parameter gradient against the fixture: the tensor's L2 norm and the seeded subset of its elements.  The subset's error
    is measured against the share of the whole tensor's norm that a subset of its size carries on average."""
    for k, grad in named_grads:
        grad = grad.detach().cpu().reshape(-1)
        want_n = float(g[f"{name}/gnorm/{k}"])
        assert float(grad.double().norm()) == pytest.approx(want_n, rel=GREL), k
        idx = W.sample_index(k, grad.numel())
        want = torch.from_numpy(g[f"{name}/gsample/{k}"]).double()
        scale = want_n * (len(idx) / grad.numel()) ** 0.5
        d = float((grad[idx].double() - want).norm()) / max(scale, 1e-30)
        assert d < GREL, (k, d)


_ORACLE = {}


def oracle_terms(use_pose, inputs, targets, eps, masks, pose_multiplier, loss_mask=None, key=None):
    """(prm, rec [B], kl [P][B]) of the reference schedule restated with the oracle's layers, with the autograd graph behind them:
    rec = the per-sample reconstruction terms summed over the subset passes, kl = each pass's per-sample KL.  Computed once per
    ``key`` and shared by the cases that differ in the KL mode or the weights only."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    prm, buf = O.split_state(seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=use_pose), 0))
    eps_it, mask_it = iter(eps), iter(masks)
    rec, kls = 0, []
    for a, b, c in (O.SUBSETS_POSE if use_pose else O.SUBSETS_NOPOSE):
        vr, tr, pr, mu, lv = O.mvae_forward(prm, inputs[0] if a else None, inputs[1] if b else None,
                                            inputs[2] if c else None, next(eps_it), mask_it, use_pose, buf)
        for on, r, x in ((a, vr, targets[0]), (b, tr, targets[1])):
            if on:
                if loss_mask is not None:
                    r, x = r * loss_mask, x * loss_mask
                rec = rec + F.binary_cross_entropy_with_logits(r, x, reduction="none").sum((1, 2, 3))
        if c:
            rec = rec + pose_multiplier * F.mse_loss(pr, targets[2], reduction="none").sum(1)
        kls.append(-0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(1))
    out = (prm, rec, torch.stack(kls))
    if key is not None:
        _ORACLE.clear()                # (one entry: the cases that share it run next to each other)
        _ORACLE[key] = out
    return out


def oracle_rows(use_pose, inputs, targets, eps, masks, kl_weight, pose_multiplier, kl, loss_mask=None, key=None):
    """(prm, rows [B]): rec plus kl_weight times the batch-total (``kl="batch"``) or the sample's own (``"sample"``) KL of every pass."""
    prm, rec, kls = oracle_terms(use_pose, inputs, targets, eps, masks, pose_multiplier, loss_mask, key)
    klb = kls if kl == "sample" else kls.sum(1, keepdim=True).expand_as(kls)
    return prm, rec + kl_weight * klb.sum(0)


def oracle_grads(prm, loss):
    keys = list(prm)
    return dict(zip(keys, torch.autograd.grad(loss, [prm[k] for k in keys], retain_graph=True)))


def engine_grads(device, use_pose, inputs, targets, eps, masks, kl_weight, w, kl, loss_mask=None, precision=None, **kw):
    """One weighted forward + backward of a fresh engine on seeded weights: (step, loss, {name: gradient})."""
    m = TM.build("cnn-mvae", True, use_pose, device)
    step = MVAEStep(m, pose_multiplier=C.POSE_MULTIPLIER, noise=InjectedNoise(eps, masks),
                    **({} if precision is None else {"precision": precision}), **kw)
    dv = lambda t: None if t is None else t.to(device)
    loss = step.forward([dv(x) for x in inputs], [dv(x) for x in targets], kl_weight, train=True, loss_mask=dv(loss_mask),
                        sample_weight=dv(w), kl=kl)
    loss = float(loss)
    partials, rows = step.partials[:step.P].clone(), None if step.last_rows is None else dict(step.last_rows)
    step.backward()
    grads = {k: (p.grad / step.loss_scale).clone() for k, p in m.named_parameters()}
    return step, loss, partials, rows, grads


def check_engine_fixture(golden_dir, device, name, precision=None):
    g = load(golden_dir, "weighted_elbo.npz")
    use_pose, B, mask_c, _ = C.MVAE_CASES[name]
    inputs, targets, eps, masks, mask, _ = C.mvae_case(name)
    w = torch.from_numpy(g[name + "/w"])
    assert torch.equal(w, W.weights(B))
    step, loss, _, rows, grads = engine_grads(device, use_pose, inputs, targets, eps, masks, C.KL_WEIGHT, w, "batch", mask, precision)
    print(name, "weighted loss", loss, "reference", float(g[name + "/loss"]))
    assert loss == pytest.approx(float(g[name + "/loss"]), rel=REL)
    np.testing.assert_allclose(rows["rows"].cpu().numpy(), g[name + "/rows"], rtol=REL)
    check_fixture_grads(g, name, grads.items())
    step.close()


def check_module_fixture(golden_dir, device, name):
    g = load(golden_dir, "weighted_elbo.npz")
    prob, x, t = TR.mvae_problem(name, device, fused=False)
    B = C.MVAE_CASES[name][1]
    w = torch.from_numpy(g[name + "/w"]).to(device)
    _, rows = prob._evaluate_model(x, t, reduce=False)
    assert rows.requires_grad and rows.dtype == torch.float32
    np.testing.assert_allclose(rows.detach().cpu().numpy(), g[name + "/rows"], rtol=REL)
    loss = (w * rows).sum() / B
    assert float(loss) == pytest.approx(float(g[name + "/loss"]), rel=REL)
    prob.model.zero_grad()
    loss.backward()
    check_fixture_grads(g, name, [(k, p.grad) for k, p in prob.model.named_parameters()])
    # rows.backward(w / B) is the same gradient
    prob2, x2, t2 = TR.mvae_problem(name, device, fused=False)
    _, rows2 = prob2._evaluate_model(x2, t2, reduce=False)
    rows2.backward(w / B)
    for (k, p1), (_, p2) in zip(prob.model.named_parameters(), prob2.model.named_parameters()):
        assert rel_l2(p2.grad, p1.grad) < 1e-5, k
    with torch.no_grad():
        prob.model.noise = InjectedNoise(*C.mvae_case(name)[2:4])
        _, r0 = prob._evaluate_model(x, t, reduce=False)
    assert not r0.requires_grad


def check_vae_fixture(golden_dir, device):
    g = load(golden_dir, "weighted_elbo.npz")
    name = W.VAE_NAME
    x, y, eps, masks, mask = C.vae_case(name)
    prob = SeqModeling(TM.args(model_name="cnn-vae", input_type="visual", use_pose=False, mask_loss=mask is not None,
                               no_cuda=(device == "cpu")), log_dir=TM.LOG_DIR, fused=False)
    m = prob.model
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    prob._kl_weight = C.KL_WEIGHT
    m.noise = InjectedNoise(eps, masks)
    _, rows = prob._evaluate_model({"model_input": x.to(device), "shock": None}, {"target_output": y.to(device), "loss_mask": mask},
                                   reduce=False)
    assert rows.requires_grad
    w = torch.from_numpy(g[name + "/w"]).to(device)
    loss = (w * rows).sum() / C.VAE_BATCH
    assert float(loss) == pytest.approx(float(g[name + "/loss"]), rel=REL)
    m.zero_grad()
    loss.backward()
    check_fixture_grads(g, name, [(k, p.grad) for k, p in m.named_parameters()])


def check_ones_equals_unweighted(device, use_pose, B=3, precision=None, mask_c=0, rel=1e-5):
    """w = 1, kl="sample": the loss, partials and gradients of the unweighted step on the same noise."""
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass, n_mask, 4321)
    mask = C.loss_mask(B, mask_c) if mask_c else None
    s0, l0, p0, r0, g0 = engine_grads(device, use_pose, inputs, targets, eps, masks, 0.3, None, "batch", mask, precision)
    s1, l1, p1, r1, g1 = engine_grads(device, use_pose, inputs, targets, eps, masks, 0.3, torch.ones(B), "sample", mask, precision)
    assert r0 is None and r1 is not None
    assert l1 == pytest.approx(l0, rel=rel)
    np.testing.assert_allclose(p1.cpu().numpy(), p0.cpu().numpy(), rtol=rel)
    assert float(r1["rows"].double().sum()) / B == pytest.approx(l0, rel=1e-5)
    worst = max(rel_l2(g1[k], g0[k]) for k in g0)
    print("w = 1 against the unweighted step: worst gradient difference", worst)
    assert worst <= rel
    s0.close(), s1.close()
    return worst


def check_linearity(device, use_pose=False, B=3, kl="sample"):
    """The gradient is linear in w: G(w1) + G(w2) against G(w1 + w2) (fresh engines, the same noise)."""
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass, n_mask, 4321)
    w1, w2 = W.weights(B, 5), W.weights(B, 6).flip(0)
    res = [engine_grads(device, use_pose, inputs, targets, eps, masks, 0.3, w, kl) for w in (w1, w2, w1 + w2)]
    assert res[0][1] + res[1][1] == pytest.approx(res[2][1], rel=1e-4)
    for k in res[0][4]:
        want = res[2][4][k]
        d = float((res[0][4][k].double() + res[1][4][k].double() - want.double()).norm()) / \
            (float(res[0][4][k].double().norm() + res[1][4][k].double().norm()) + 1e-30)
        assert d < 1e-4, (k, d)
    for r in res:
        r[0].close()


def check_engine_vs_oracle(device, use_pose, B, kl, precision=None, mask_c=0, skip=()):
    """MVAEStep against the autograd restatement: loss / partials-sum 1e-4, rows 1e-4, every gradient tensor 1e-3 relative L2."""
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass, n_mask, 4321)
    mask = C.loss_mask(B, mask_c) if mask_c else None
    w = W.weights(B)
    prm, rows_o = oracle_rows(use_pose, inputs, targets, list(eps), list(masks), 0.3, C.POSE_MULTIPLIER, kl, mask,
                              key=(use_pose, B, mask_c))
    loss_o = (w * rows_o).sum() / B
    og = oracle_grads(prm, loss_o)
    step, loss, partials, rows, grads = engine_grads(device, use_pose, inputs, targets, eps, masks, 0.3, w, kl, mask, precision)
    print("B", B, kl, precision, "loss", loss, "oracle", float(loss_o))
    assert loss == pytest.approx(float(loss_o), rel=REL)
    assert float(partials.double().sum()) == pytest.approx(float(loss_o), rel=REL)
    np.testing.assert_allclose(rows["rows"].cpu().numpy(), rows_o.detach().numpy(), rtol=REL)
    worst = {}
    for k, gr in grads.items():
        worst[k] = rel_l2(gr.cpu(), og[k])
    bad = {k: v for k, v in worst.items() if v >= GREL and k not in skip}
    print("worst gradient tensor", max(worst.items(), key=lambda kv: kv[1]))
    assert not bad, bad
    step.close()


def check_train_batch(device, fused):
    """Problem.train_batch: loader-format lists in, one optimiser step, {"loss", "rows"} out; w = None is w = 1."""
    inputs, targets, eps, masks, _, _ = C.mvae_case("pose")
    out = {}
    for w in (None, W.weights(4)):
        prob = SeqModeling(TM.args(no_cuda=(device == "cpu")), log_dir=TM.LOG_DIR, fused=fused)
        assert (prob._step is not None) == fused
        prob.model.load_state_dict(seeded_state_dict(prob.model.state_dict(), 0))
        prob._kl_weight = C.KL_WEIGHT
        prob.model.noise = InjectedNoise(eps, masks)
        if prob._step is not None:
            # (on the GPU the fused step is captured into graphs: the warm-up and the capture both draw, so the Philox source)
            prob._step.noise = InjectedNoise(eps, masks) if device == "cpu" else NoiseSource(7)
        before = {k: p.detach().clone() for k, p in prob.model.named_parameters()}
        data = list(inputs) + [torch.ones(4, 2)]
        target = list(targets) + [torch.ones(4, 1, 64, 64)]
        res = prob.train_batch(data, target, sample_weight=None if w is None else w.to(device), kl="sample")
        assert set(res) == {"loss", "rows"} and res["rows"].shape == (4,) and res["loss"].dim() == 0
        assert not res["rows"].requires_grad and not res["loss"].requires_grad
        ww = torch.ones(4) if w is None else w
        assert float(res["loss"]) == pytest.approx(float((ww.double() * res["rows"].double().cpu()).sum()) / 4, rel=1e-5)
        moved = sum(int(not torch.equal(before[k], p.detach())) for k, p in prob.model.named_parameters())
        assert moved == len(before)
        out[w is None] = res
        with pytest.raises(ValueError):
            prob.train_batch(data, target, kl="mean")
        if prob._step is not None:
            prob._step.close()
    return out


# ---- the tests (CPU, emulation backend) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.MVAE_NAMES)
def test_fixture_fused_engine(golden_dir, name):
    check_engine_fixture(golden_dir, "cpu", name)


@pytest.mark.parametrize("name", W.MVAE_NAMES)
def test_fixture_module_api(golden_dir, name):
    check_module_fixture(golden_dir, "cpu", name)


def test_fixture_vae_module_api(golden_dir):
    check_vae_fixture(golden_dir, "cpu")


@pytest.mark.parametrize("use_pose,mask_c", [(True, 0), (False, 1)])
def test_ones_equals_unweighted_engine(use_pose, mask_c):
    check_ones_equals_unweighted("cpu", use_pose, mask_c=mask_c)


def test_ones_equals_unweighted_module_api():
    """kl="sample" rows with w = 1 through the module API: the scalar loss and its gradients."""
    name = "nopose"
    prob, x, t = TR.mvae_problem(name, "cpu", fused=False)
    _, loss = prob._evaluate_model(x, t)
    loss.backward()
    prob2, x2, t2 = TR.mvae_problem(name, "cpu", fused=False)
    prob2._rows_kl_mode = 1
    _, rows = prob2._evaluate_model(x2, t2, reduce=False)
    (rows.sum() / rows.shape[0]).backward()
    assert float(rows.sum()) / rows.shape[0] == pytest.approx(float(loss), rel=1e-5)
    for (k, p1), (_, p2) in zip(prob.model.named_parameters(), prob2.model.named_parameters()):
        assert rel_l2(p2.grad, p1.grad) < 1e-5, k


def test_linearity_engine():
    check_linearity("cpu")


def test_linearity_module_api():
    name, B = "nopose", 4
    w1, w2 = W.weights(B, 5), W.weights(B, 6).flip(0)
    grads = []
    for w in (w1, w2, w1 + w2):
        prob, x, t = TR.mvae_problem(name, "cpu", fused=False)
        _, rows = prob._evaluate_model(x, t, reduce=False)
        rows.backward(w / B)
        grads.append({k: p.grad.clone() for k, p in prob.model.named_parameters()})
    for k in grads[0]:
        assert rel_l2(grads[0][k] + grads[1][k], grads[2][k]) < 1e-4, k


@pytest.mark.parametrize("use_pose,kl", [(True, "sample"), (True, "batch"), (False, "sample")])
def test_engine_vs_oracle(use_pose, kl):
    check_engine_vs_oracle("cpu", use_pose, 3, kl, mask_c=0 if use_pose else 3)


def test_module_api_kl_sample_vs_oracle():
    name = "pose"
    use_pose, B = C.MVAE_CASES[name][:2]
    inputs, targets, eps, masks, _, _ = C.mvae_case(name)
    w = W.weights(B)
    prm, rows_o = oracle_rows(use_pose, inputs, targets, list(eps), list(masks), C.KL_WEIGHT, C.POSE_MULTIPLIER, "sample")
    og = oracle_grads(prm, (w * rows_o).sum() / B)
    prob, x, t = TR.mvae_problem(name, "cpu", fused=False)
    prob._rows_kl_mode = 1
    _, rows = prob._evaluate_model(x, t, reduce=False)
    np.testing.assert_allclose(rows.detach().numpy(), rows_o.detach().numpy(), rtol=REL)
    ((w * rows).sum() / B).backward()
    for k, p in prob.model.named_parameters():
        assert rel_l2(p.grad, og[k]) < GREL, k


def test_exact_running_stats_with_weights():
    """The discarded passes (slot < 0) take a zero gradient and no loss in the weighted launches too: same loss and gradients."""
    B = 2
    inputs, targets = seeded_batch(B, 1234, with_pose=True)
    w = W.weights(B)
    res = []
    for exact in (False, True):
        eps, masks = seeded_noise(B, 256, 7, 8, 4321)
        res.append(engine_grads("cpu", True, inputs, targets, eps, masks, 0.3, w, "sample", exact_running_stats=exact))
    assert res[1][1] == pytest.approx(res[0][1], rel=1e-5)
    for k in res[0][4]:
        assert rel_l2(res[1][4][k], res[0][4][k]) < 1e-4, k


@pytest.mark.parametrize("fused", [False, True])
def test_train_batch(fused):
    out = check_train_batch("cpu", fused)
    # the rows of the batch do not depend on the weights
    np.testing.assert_allclose(out[True]["rows"].cpu().numpy(), out[False]["rows"].cpu().numpy(), rtol=1e-6)


def test_value_errors():
    inputs, targets = seeded_batch(2, 1234, with_pose=False)
    m = TM.build("cnn-mvae", True, False, "cpu")
    step = MVAEStep(m)
    with pytest.raises(ValueError):
        step.forward(inputs, targets, 1.0, sample_weight=torch.ones(2), kl="mean")
    with pytest.raises(ValueError):
        step.forward(inputs, targets, 1.0, sample_weight=torch.ones(3))
    with pytest.raises(ValueError):
        step.forward(inputs, targets, 1.0, sample_weight=torch.ones(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        step.forward(inputs, targets, 1.0, train=False, rows=True, sample_weight=torch.ones(2))
    step.pg = object()               # a process group: data-parallel weighting is not built
    with pytest.raises(ValueError, match="not built"):
        step.train_step(inputs, targets, 1.0, sample_weight=torch.ones(2))
    step.pg = None
    # HipBackend checks the weight vector before it touches the library
    with pytest.raises(ValueError):
        ops.HipBackend._weights(torch.ones(3), 2, "t")
    with pytest.raises(ValueError):
        ops.HipBackend._weights(torch.ones(2, dtype=torch.float64), 2, "t")
    step.close()


def test_eval_step_with_weights():
    B = 3
    inputs, targets = seeded_batch(B, 1234, with_pose=False)
    eps, masks = seeded_noise(B, 256, 3, 4, 4321)
    w = W.weights(B)
    m = TM.build("cnn-mvae", True, False, "cpu")
    step = MVAEStep(m, noise=InjectedNoise(eps, masks))
    loss = float(step.eval_step(inputs, targets, 0.3, sample_weight=w, kl="sample"))
    rows = step.last_rows["rows"].double()
    assert loss == pytest.approx(float((w.double() * rows).sum()) / B, rel=1e-5)
    step.close()


def test_backend_without_the_weighted_ops_is_an_error():
    """A backend from before the weighted ops keeps its forward; the backward of its rows and a weighted engine step name the
    missing op in a RuntimeError (ops.backend_op) -- no fallback."""
    from emu_backend_rows import EmuBackendRows
    old = ops.set_backend(EmuBackendRows())
    try:
        prob, x, t = TR.mvae_problem("nopose", "cpu", fused=False)
        _, rows = prob._evaluate_model(x, t, reduce=False)
        assert rows.requires_grad
        with pytest.raises(RuntimeError, match="has no op 'reparam_bwd_weighted'"):
            rows.sum().backward()
        step = MVAEStep(prob.model)
        with pytest.raises(RuntimeError, match="has no op"):
            step.train_step(x["model_input"], t["target_output"], 1.0, sample_weight=torch.ones(C.MVAE_CASES["nopose"][1]))
        step.close()
    finally:
        ops.set_backend(old)
    assert ops.backend_op("reparam_bwd_weighted") is not None
