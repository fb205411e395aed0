"""Per-sample ELBO (``reduce=False``) on the CPU: the Problem API, the module API and the fused engine's ``score_step`` through the
emulation backend (tests/emu_backend_rows.py) against tests/golden/elbo_rows.npz -- the reference's own rows on the seeded cases
of tests/rows_cases.py -- and the scalar (``reduce=None``) path unchanged under the same backend."""
import numpy as np
import pytest
import torch

import rows_cases as C
import test_model_emu as TM
from emu_backend_rows import EmuBackendRows
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import setup_model, InjectedNoise
from mmdyn_hip.problems.problems import SeqModeling
from mmdyn_hip.utils.seeded_init import seeded_state_dict
from test_oracle_golden import load

# the relative tolerance tests/test_model_emu.py applies to the scalar loss and its per-pass partials against the reference
REL = 1e-4


@pytest.fixture(autouse=True)
def emu_rows():
    old = ops.set_backend(EmuBackendRows())
    yield
    ops.set_backend(old)


def mvae_problem(name, device, fused):
    """(problem, x, targets) of one cnn-mvae case, in the dict format of SeqModeling.parse_input."""
    use_pose, B, mask_c, conditional = C.MVAE_CASES[name]
    inputs, targets, eps, masks, mask, cond = C.mvae_case(name)
    if conditional:
        kw = dict(TM.MODEL_KW)
        kw.update(conditional=True, condition_dim=3, use_pose=True)
        m = setup_model("cnn-mvae", cross_modal=True, **kw)
        m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
        m.to(device).train()
        prob = SeqModeling.__new__(SeqModeling)
        prob._model, prob._kl_weight, prob._pose_multiplier, prob._conditional = m, C.KL_WEIGHT, C.POSE_MULTIPLIER, True
        prob._step = MVAEStep(m, pose_multiplier=C.POSE_MULTIPLIER) if fused else None
        prob.parameters = {"use_pose": True, "model_name": "cnn-mvae", "mask_loss": False, "input_type": "visuotactile"}
    else:
        prob = SeqModeling(TM.args(use_pose=use_pose, mask_loss=mask is not None, no_cuda=(device == "cpu"),
                                   pose_multiplier=C.POSE_MULTIPLIER), log_dir=TM.LOG_DIR, fused=fused)
        m = prob.model
        m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
        prob._kl_weight = C.KL_WEIGHT
    noise = InjectedNoise(eps, masks)
    m.noise = noise
    if prob._step is not None:
        prob._step.noise = noise
    dv = lambda t: None if t is None else t.to(device)
    x = {"model_input": [dv(inputs[0]), dv(inputs[1])], "input_object_pose": [dv(inputs[2])] if use_pose else None,
         "shock": dv(cond)}
    t = {"target_output": [dv(targets[0]), dv(targets[1])], "target_object_pose": [dv(targets[2])] if use_pose else None,
         "loss_mask": dv(mask)}
    return prob, x, t


def check_mvae_rows_module_api(golden_dir, device, name):
    """The reference's schedule (one model call per subset) with reduce=False: rows, per-pass rows and the outputs dict."""
    g = load(golden_dir, "elbo_rows.npz")
    prob, x, t = mvae_problem(name, device, fused=False)
    assert prob._step is None
    passes, inner = [], prob._mvae_elbo_loss
    prob._mvae_elbo_loss = lambda *a, **k: (passes.append(inner(*a, **k)), passes[-1])[1]
    with torch.no_grad():
        outputs, rows = prob._evaluate_model(x, t, reduce=False)
    B = C.MVAE_CASES[name][1]
    assert rows.shape == (B,) and rows.dtype == torch.float32 and not rows.requires_grad
    print(name, "rows", rows.cpu().numpy(), "reference", g[name + "/rows"])
    np.testing.assert_allclose(rows.cpu().numpy(), g[name + "/rows"], rtol=REL)
    np.testing.assert_allclose(torch.stack(passes).cpu().numpy(), g[name + "/pass_rows"], rtol=REL)
    np.testing.assert_allclose(outputs["means"].cpu().numpy(), g[name + "/means"], rtol=1e-4, atol=3e-5)
    assert set(outputs) == {"recon_x", "means", "log_var", "perf_measure"}
    # the quirk the rows carry: the batch-total KL sits in every row, so their mean is not the scalar loss
    # (each row exceeds its share of the scalar by kl_weight * the other samples' KL)
    assert float(g[name + "/rows"].mean()) > float(g[name + "/scalar"]) and float(rows.mean()) > float(g[name + "/scalar"])


def check_mvae_rows_engine(golden_dir, device, name, precision=None):
    """The same rows from the fused engine (Problem API -> MVAEStep.score_step), both KL modes and the scalar beside them."""
    g = load(golden_dir, "elbo_rows.npz")
    prob, x, t = mvae_problem(name, device, fused=True)
    step = prob._step
    assert step is not None
    if precision is not None and step.precision != precision:
        step.close()
        step = prob._step = MVAEStep(prob.model, pose_multiplier=C.POSE_MULTIPLIER, precision=precision, noise=prob.model.noise)
    use_pose, B = C.MVAE_CASES[name][:2]
    with torch.no_grad():
        outputs, rows = prob._evaluate_model(x, t, reduce=False)
    print(name, step.precision, "rows", rows.cpu().numpy(), "reference", g[name + "/rows"])
    np.testing.assert_allclose(rows.cpu().numpy(), g[name + "/rows"], rtol=REL)
    np.testing.assert_allclose(outputs["means"].cpu().numpy(), g[name + "/means"], rtol=1e-4, atol=3e-5)
    # score_step itself: per-pass rows (the engine's pass order is the reference's), the scalar of the reduce=None call, identities
    xs, ts = prob._fused_io(x, t)
    mask = t["loss_mask"] if prob.parameters["mask_loss"] else None
    res = {}
    for kl in ("batch", "sample"):
        step.noise = InjectedNoise(*C.mvae_case(name)[2:4])
        res[kl] = step.score_step(xs, ts, C.KL_WEIGHT, loss_mask=mask, condition=x["shock"], kl=kl)
    rb, rs = res["batch"], res["sample"]
    P = step.P
    np.testing.assert_allclose(rb["rows"].cpu().numpy(), g[name + "/rows"], rtol=REL)
    np.testing.assert_allclose(rb["partials"].cpu().numpy(), g[name + "/pass_rows"], rtol=REL)
    assert float(rb["loss"]) == pytest.approx(float(g[name + "/scalar"]), rel=REL)
    step.noise = InjectedNoise(*C.mvae_case(name)[2:4])
    ev = step.eval_step(xs, ts, C.KL_WEIGHT, loss_mask=mask, condition=x["shock"])
    assert float(rb["loss"]) == pytest.approx(float(ev), rel=1e-6)
    np.testing.assert_allclose(rb["loss_partials"].cpu().numpy(), step.partials[:P].cpu().numpy(), rtol=1e-6)
    assert float(rs["rows"].double().sum()) / B == pytest.approx(float(ev), rel=1e-5)
    kl_sum = rb["kl_rows"].sum(1, keepdim=True)
    want = (C.KL_WEIGHT * (kl_sum - rb["kl_rows"])).sum(0)
    np.testing.assert_allclose((rb["rows"].double() - rs["rows"].double()).cpu().numpy(), want.cpu().numpy(), rtol=1e-3, atol=0.05)
    step.close()


@pytest.mark.parametrize("name", list(C.MVAE_CASES))
def test_mvae_rows_module_api(golden_dir, name):
    check_mvae_rows_module_api(golden_dir, "cpu", name)


@pytest.mark.parametrize("name", list(C.MVAE_CASES))
def test_mvae_rows_fused_engine(golden_dir, name):
    check_mvae_rows_engine(golden_dir, "cpu", name)


def check_vae_rows(golden_dir, device, name):
    g = load(golden_dir, "elbo_rows.npz")
    x, y, eps, masks, mask = C.vae_case(name)
    prob = SeqModeling(TM.args(model_name="cnn-vae", input_type="visual", use_pose=False, mask_loss=mask is not None,
                               no_cuda=(device == "cpu")), log_dir=TM.LOG_DIR, fused=False)
    m = prob.model
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    prob._kl_weight = C.KL_WEIGHT
    for reduce in (False, None):
        m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
        m.noise = InjectedNoise(eps, masks)
        with torch.no_grad():
            out, loss = prob._evaluate_model({"model_input": x.to(device), "shock": None},
                                             {"target_output": y.to(device), "loss_mask": None if mask is None else mask.to(device)},
                                             reduce=reduce)
        if reduce is False:
            assert loss.shape == (C.VAE_BATCH,) and loss.dtype == torch.float32
            np.testing.assert_allclose(loss.cpu().numpy(), g[name + "/rows"], rtol=REL)
        else:
            assert float(loss) == pytest.approx(float(g[name + "/scalar"]), rel=REL)


@pytest.mark.parametrize("name", list(C.VAE_CASES))
def test_vae_rows(golden_dir, name):
    check_vae_rows(golden_dir, "cpu", name)


def check_score_wrapper(device):
    """Problem.score: loader-format lists in, the [B] rows out, no autograd graph."""
    inputs, targets, eps, masks, _, _ = C.mvae_case("pose")
    rows = {}
    for fused in (False, True):
        prob = SeqModeling(TM.args(no_cuda=(device == "cpu")), log_dir=TM.LOG_DIR, fused=fused)
        prob.model.load_state_dict(seeded_state_dict(prob.model.state_dict(), 0))
        prob._kl_weight = C.KL_WEIGHT
        prob.model.noise = InjectedNoise(eps, masks)
        if prob._step is not None:
            prob._step.noise = InjectedNoise(eps, masks)
        data = list(inputs) + [torch.ones(4, 2)]
        target = list(targets) + [torch.ones(4, 1, 64, 64)]
        rows[fused] = prob.score(data, target)
        assert rows[fused].shape == (4,) and not rows[fused].requires_grad
        if prob._step is not None:
            prob._step.close()
    return rows


def test_problem_score(golden_dir):
    g = load(golden_dir, "elbo_rows.npz")
    rows = check_score_wrapper("cpu")
    for r in rows.values():
        np.testing.assert_allclose(r.cpu().numpy(), g["pose/rows"], rtol=REL)


def test_what_stays_unsupported_still_raises():
    prob, x, t = mvae_problem("nopose", "cpu", fused=False)
    with pytest.raises(NotImplementedError):
        prob._evaluate_model(x, t, reduce=True)
    with pytest.raises(NotImplementedError):
        prob._evaluate_model(x, t, reduction="mean")
    with pytest.raises(NotImplementedError):
        prob._evaluate_model(x, t, reduction="none")
    prob.model.noise = InjectedNoise(*C.mvae_case("nopose")[2:4])
    _, rows = prob._evaluate_model(x, t, reduce=False)        # forward only: no graph behind the rows
    with pytest.raises(RuntimeError):
        rows.sum().backward()
    step = MVAEStep(prob.model)
    with pytest.raises(ValueError):
        step.score_step(x["model_input"], t["target_output"], 1.0, kl="mean")
    with pytest.raises(ValueError):
        step.forward(x["model_input"], t["target_output"], 1.0, train=True, rows=True)
    step.close()


def test_scalar_path_unchanged(golden_dir):
    """reduce=None under the rows backend: the existing reference-pinned checks of the scalar loss, gradients and parameters."""
    TM.check_reference_schedule_step(golden_dir, "cpu", "mvae_nopose_B4.npz", False)
    TM.check_fused_engine(golden_dir, "cpu", "mvae_pose_B4.npz", True)
    TM.check_vae_config1(golden_dir, "cpu")
    TM.check_conditional(golden_dir, "cpu")


def test_row_tables_are_validated_on_the_host():
    """HipBackend checks the row tables before it touches the library (no library call here)."""
    with pytest.raises(ValueError):
        ops.HipBackend._row_slots(torch.zeros(2, 4), 4, "t")                       # fp32 table
    with pytest.raises(ValueError):
        ops.HipBackend._row_slots(torch.zeros(2, 5, dtype=torch.float64), 4, "t")  # wrong batch
    assert ops.HipBackend._row_slots(torch.zeros(3, 4, dtype=torch.float64), 4, "t") == 3


def eval_engine(device, **kw):
    """The serving engine on the model of the eval-mode fixtures (seeded weights and running statistics, eval())."""
    from mmdyn_hip.engine import MVAEInference
    from mmdyn_hip.utils.seeded_init import seeded_running_stats
    m = TM.build("cnn-mvae", True, True, device)
    m.load_state_dict(seeded_running_stats({k: v.cpu() for k, v in m.state_dict().items()}))
    m.eval()
    return MVAEInference(m, **kw)


def check_inference_score(golden_dir, device, precision="fp32x3"):
    """MVAEInference.score: the per-sample BCE / MSE / KL of one eval-mode joint pass against the reference model's (eval/* of
    elbo_rows.npz, computed there with reduction='none'), with explicit targets and with the inputs as targets; `rows` is their
    weighted sum; a loss mask against torch on the returned logits; subsets; argument errors."""
    g = load(golden_dir, "elbo_rows.npz")
    inputs, targets, eps = C.eval_case()
    inputs, targets = [x.to(device) for x in inputs], [x.to(device) for x in targets]
    eng = eval_engine(device, precision=precision)
    eng.use_graph = False                                   # injected noise: compare with the reference's vectors
    klw, pm = 0.3, 1000.0
    for pre, tg in (("eval/", targets), ("eval/self_", None)):
        eng.noise = InjectedNoise([eps.clone()], [])
        r = eng.score([inputs[0], inputs[1]], pose=inputs[2], targets=tg, kl_weight=klw, pose_multiplier=pm)
        got = {k: r[k].double().cpu().numpy() for k in ("bce_visual", "bce_tactile", "mse_pose", "kl", "rows")}
        print(pre, {k: v for k, v in got.items()})
        for k in ("bce_visual", "bce_tactile", "mse_pose"):
            np.testing.assert_allclose(got[k], g[pre + k], rtol=REL)
        np.testing.assert_allclose(got["kl"], g["eval/kl"], rtol=REL)
        want = (g[pre + "bce_visual"].astype(np.float64) + g[pre + "bce_tactile"] + pm * g[pre + "mse_pose"].astype(np.float64)
                + klw * g["eval/kl"].astype(np.float64))
        np.testing.assert_allclose(got["rows"], want, rtol=REL)
        assert r["rows"].dtype == torch.float32 and tuple(r["rows"].shape) == (C.EVAL_BATCH,)
    # visual only, masked: against torch on the logits the call returns
    import torch.nn.functional as F
    mask = C.loss_mask(C.EVAL_BATCH, 1).to(device)
    eng.noise = InjectedNoise([eps.clone()], [])
    r = eng.score([inputs[0], None], targets=[targets[0], None, None], loss_mask=mask, kl_weight=klw)
    assert r["bce_tactile"] is None and r["mse_pose"] is None
    lg = r["recon_x"][0].double()
    want = F.binary_cross_entropy_with_logits(lg * mask.double(), targets[0].double() * mask.double(), reduction="none").sum((1, 2, 3))
    np.testing.assert_allclose(r["bce_visual"].cpu().numpy(), want.cpu().numpy(), rtol=1e-5)
    np.testing.assert_allclose(r["rows"].double().cpu().numpy(), (want + klw * r["kl"]).cpu().numpy(), rtol=1e-6)
    with pytest.raises(ValueError):
        eng.score([inputs[0], inputs[1]], pose=inputs[2], loss_mask=mask)
    with pytest.raises(ValueError):
        eng.score([None, None])
    with pytest.raises(ValueError):
        eng.score([inputs[0], None], targets=[targets[0][:2], None, None])
    eng.close()


def test_inference_score(golden_dir):
    check_inference_score(golden_dir, "cpu")
