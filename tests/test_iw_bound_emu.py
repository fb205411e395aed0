"""Importance-weighted K-sample bound on the CPU: ``MVAEInference.score(samples=K)`` through the emulation backend
(tests/emu_backend_iw.py) against the fp64 restatement on the oracle's eval-mode forward functions (tests/iw_cases.py) -- the
reference has no such estimator, so there is no golden file --, the untouched ``samples=None`` path, the launch count, the error
paths and ``Reconstruction.iw_score``.  The ``check_*`` functions take the device: tests/test_iw_bound_gpu.py runs them on the HIP
library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cond_cases as CC
import iw_cases as IW
import test_mixed_modal_emu as TMM
import test_model_emu as TM
from emu_backend_evalgrad import EmuBackendEvalGrad
from emu_backend_iw import EmuBackendIW, Recorder
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.problems.problems import SeqModeling
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_state_dict
from test_elbo_rows_emu import REL          # engine rows against the oracle: the bound that file and its GPU twin apply

KL_WEIGHT, POSE_MULTIPLIER = 0.3, 1000.0
L = CC.LATENT
# row b holds MIXED[b] of (visual, tactile, pose): joint, one image, nothing (the prior alone), two modalities, the pose alone
MIXED = [(1, 1, 1), (1, 0, 0), (0, 0, 0), (0, 1, 1), (0, 0, 1)]
# name -> (B, K, categorical condition)
CASES = {"joint": (5, 3, False), "visual_targets": (2, 4, False), "mixed": (5, 2, False), "categorical": (3, 2, True),
         "mask1": (3, 2, False)}


@pytest.fixture(autouse=True)
def emu_iw():
    old = ops.set_backend(EmuBackendIW())
    yield
    ops.set_backend(old)


def request(name):
    """(B, K, categorical, keyword arguments of score() on CPU tensors, eps [K][B][L]) of one case."""
    B, K, categorical = CASES[name]
    inputs, targets = seeded_batch(B, 700 + len(name), with_pose=True)
    eps = torch.randn(K, B, L, generator=torch.Generator().manual_seed(70 + B + K))
    kw = dict(x=[inputs[0], inputs[1]], pose=inputs[2], kl_weight=KL_WEIGHT, pose_multiplier=POSE_MULTIPLIER)
    if name == "visual_targets":
        kw.update(x=[inputs[0], None], pose=None, targets=[targets[0], None, None])
    elif name == "mixed":
        kw.update(available=torch.tensor(MIXED, dtype=torch.float64))
    elif name == "categorical":
        kw.update(condition=CC.indices(B, 27))
    elif name == "mask1":
        kw.update(pose=None, loss_mask=(torch.rand(B, 1, 64, 64, generator=torch.Generator().manual_seed(5)) < 0.7).float())
    return B, K, categorical, kw, eps


def restate(model, kw, eps, categorical):
    prm, buf = IW.oracle_state(model)
    x, pose = kw["x"], kw.get("pose")
    targets = kw.get("targets") or [x[0], x[1], pose]
    av = kw.get("available")
    cond = kw.get("condition")
    if cond is not None and categorical:
        cond = F.one_hot(cond, CC.CAT_DIM).float()
    return IW.iw_request_ref(prm, buf, [x[0], x[1], pose], targets, eps, kw["kl_weight"], kw["pose_multiplier"], available=av,
                             target_available=av if kw.get("targets") is None else None, cond=cond, loss_mask=kw.get("loss_mask"))


def to_device(kw, device):
    mv = lambda t: t.to(device) if torch.is_tensor(t) else ([None if u is None else u.to(device) for u in t] if isinstance(t, list) else t)
    return {k: mv(v) for k, v in kw.items()}


def check_engine_case(device, name, precision="fp32x3"):
    """score(samples=K), eager, injected noise: the per-draw terms, the density ratios, the weights and the bound against the
    restatement on the oracle (REL, the bound of the engine-versus-oracle row comparisons); the effective sample size against the
    definition applied to the call's own tables; the per-draw terms against today's score() called once per draw with that draw
    injected; shapes, dtypes and which entries are None."""
    B, K, categorical, kw, eps = request(name)
    model = TMM.build(categorical, device)
    eng = MVAEInference(model, precision=precision, use_graph=False)
    want = restate(model, kw, eps, categorical)
    dkw = to_device(kw, device)
    x = dkw.pop("x")
    eng.noise = InjectedNoise([eps.clone()], [])
    r = eng.score(x, samples=K, **dkw)
    assert set(r) == {"rows", "ess", "log_w", "ratio", "bce_visual", "bce_tactile", "mse_pose", "kl", "means", "log_var", "recon_x"}
    assert r["rows"].dtype == torch.float32 and tuple(r["rows"].shape) == (B,) and tuple(r["ess"].shape) == (B,)
    assert tuple(r["recon_x"][0].shape) == (K * B, 3, 64, 64) and tuple(r["means"].shape) == (B, L)
    np.testing.assert_allclose(r["means"].cpu().numpy(), want["means"].numpy(), **TMM.OUT_TOL)
    np.testing.assert_allclose(r["log_var"].cpu().numpy(), want["log_var"].numpy(), **TMM.OUT_TOL)
    for k in ("bce_visual", "bce_tactile", "mse_pose", "ratio", "log_w"):
        if want[k] is None:
            assert r[k] is None, k
            continue
        assert r[k].dtype == torch.float64 and tuple(r[k].shape) == (K, B), k
        got, ref = r[k].cpu().numpy(), want[k].numpy()
        print(name, precision, k, "largest relative deviation", float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))))
        np.testing.assert_allclose(got, ref, rtol=REL, err_msg=k)
    np.testing.assert_allclose(r["kl"].cpu().numpy(), want["kl"].numpy(), rtol=REL)
    print(name, precision, "rows", r["rows"].cpu().numpy(), "restatement", want["rows"].numpy(), "ess", r["ess"].cpu().numpy())
    np.testing.assert_allclose(r["rows"].double().cpu().numpy(), want["rows"].numpy(), rtol=REL)
    # the sample size: the definition on the weights this call published (fp32 result of an fp64 expression)
    lw = r["log_w"].cpu()
    ess = torch.exp(2.0 * torch.logsumexp(lw, 0) - torch.logsumexp(2.0 * lw, 0))
    np.testing.assert_allclose(r["ess"].double().cpu().numpy(), ess.numpy(), rtol=1e-6)
    assert float(r["ess"].min()) >= 1.0 and float(r["ess"].max()) <= K
    # ... and the draws one by one through the path that exists today
    got = {k: (None if r[k] is None else r[k].clone()) for k in ("bce_visual", "bce_tactile", "mse_pose", "means", "kl")}
    for k in range(K):
        eng.noise = InjectedNoise([eps[k].clone()], [])
        one = eng.score(x, **dkw)
        assert torch.equal(one["means"], got["means"]) and torch.equal(one["kl"], got["kl"])
        for term in ("bce_visual", "bce_tactile", "mse_pose"):
            if got[term] is None:
                assert one[term] is None
            else:
                np.testing.assert_allclose(got[term][k].cpu().numpy(), one[term].cpu().numpy(), rtol=REL, err_msg=f"{term} draw {k}")
    eng.close()
    return r, want


@pytest.mark.parametrize("name", list(CASES))
def test_score_samples_against_the_restatement(name):
    r, want = check_engine_case("cpu", name)
    if name == "mixed":
        on = torch.tensor(MIXED, dtype=torch.bool)
        for m, term in enumerate(("bce_visual", "bce_tactile", "mse_pose")):
            assert float(r[term][:, ~on[:, m]].abs().max()) == 0.0 and float(r[term][:, on[:, m]].min()) > 0.0
        # the row that holds nothing: no reconstruction term, the weights are the prior-to-posterior ratios alone
        np.testing.assert_allclose(r["log_w"][:, 2].numpy(), -KL_WEIGHT * r["ratio"][:, 2].numpy(), rtol=1e-12)
        assert torch.equal(r["means"][2], torch.zeros(L))


def test_one_draw_is_the_single_sample_bound():
    """K = 1: rows = rec_0 + kl_weight * ratio_0 (fp32 rounding of the fp64 sum) and ess = 1, exactly."""
    B, _, _, kw, _ = request("joint")
    eps = torch.randn(1, B, L, generator=torch.Generator().manual_seed(3))
    eng = MVAEInference(TMM.build(False), use_graph=False)
    eng.noise = InjectedNoise([eps], [])
    x = kw.pop("x")
    r = eng.score(x, samples=1, **kw)
    rec = r["bce_visual"][0] + r["bce_tactile"][0] + POSE_MULTIPLIER * r["mse_pose"][0]
    klw = float(torch.tensor(1.0) * torch.tensor(KL_WEIGHT))          # (the fp32 weight the assembly reads from device memory)
    assert torch.equal(r["rows"], (rec + klw * r["ratio"][0]).float())
    assert torch.equal(r["ess"], torch.ones(B))
    eng.close()


OLD_KEYS = {"rows", "bce_visual", "bce_tactile", "mse_pose", "kl", "recon_x", "means", "log_var"}


def test_without_samples_nothing_changes():
    """samples=None: the ops of the request in call order -- one PoE launch with z, the four row-kernel launches and the assembly
    of the per-sample ELBO, no iw op -- on a backend that has the new ops and on one that does not, with equal results."""
    B, _, _, kw, _ = request("joint")
    eps = torch.randn(B, L, generator=torch.Generator().manual_seed(4))
    x = kw.pop("x")
    runs = []
    for backend in (EmuBackendEvalGrad(), EmuBackendIW()):
        rec = Recorder(backend)
        ops.set_backend(rec)
        eng = MVAEInference(TMM.build(False), use_graph=False)
        del rec.ops[:]
        eng.noise = InjectedNoise([eps.clone()], [])
        r = eng.score(x, **kw)
        assert set(r) == OLD_KEYS
        runs.append((list(rec.ops), {k: v.clone() for k, v in r.items() if torch.is_tensor(v)}, [t.clone() for t in r["recon_x"]]))
        eng.close()
    (ops_a, res_a, rx_a), (ops_b, res_b, rx_b) = runs
    assert ops_a == ops_b and not any(o.startswith("iw_") for o in ops_a)
    assert ops_a.count("poe_fwd") == 1
    assert ops_a[-5:] == ["bce_logits_rows_groups", "bce_logits_rows_groups", "mse_rows_groups", "kl_rows", "elbo_assemble_rows"]
    for k in res_a:
        assert torch.equal(res_a[k], res_b[k]), k
    assert all(torch.equal(a, b) for a, b in zip(rx_a, rx_b))


def recorded_ops(K, name="joint"):
    B, _, _, kw, _ = request(name)
    x = kw.pop("x")
    rec = Recorder(EmuBackendIW())
    ops.set_backend(rec)
    eng = MVAEInference(TMM.build(False), use_graph=False)
    del rec.ops[:]
    eng.score(x, samples=K, **kw)
    eng.close()
    return list(rec.ops)


def test_launch_count_does_not_depend_on_the_number_of_draws():
    one, four = recorded_ops(1), recorded_ops(4)
    assert one == four
    assert one.count("poe_fwd") == 1 and one.count("iw_latent") == 1 and one.count("iw_assemble_rows") == 1
    assert one.count("random_normal") == 1 and one.count("counter_add") == 1          # one draw, then the commit
    assert one.count("bce_logits_rows_groups") == 2 and one.count("mse_rows_groups") == 1 and "elbo_assemble_rows" not in one
    # past the row kernels' MMDYN_BCE_GROUPS_MAX = 8 passes per launch: one more launch per term, the rest as before
    nine = recorded_ops(9)
    assert nine.count("bce_logits_rows_groups") == 4 and nine.count("mse_rows_groups") == 2
    assert [o for o in nine if "rows_groups" not in o] == [o for o in one if "rows_groups" not in o]


def test_argument_errors():
    B, _, _, kw, _ = request("joint")
    x = kw.pop("x")
    eng = MVAEInference(TMM.build(False), use_graph=False)
    for bad in (0, -2, 2.0, 2.5, "3", True):
        with pytest.raises(ValueError, match="samples"):
            eng.score(x, samples=bad, **kw)
    # K * B * 32 * 32 * 32 >= 2^31: refused up front, and the message says how far one may go
    most = (2 ** 31 - 1) // (B * 32 * 32 * 32)
    assert (most + 1) * B * 32768 >= 2 ** 31 > most * B * 32768
    with pytest.raises(ValueError, match=rf"largest samples for B = {B} is {most}\b"):
        eng.score(x, samples=most + 1, **kw)
    # a backend written before the ops: an error that names the op, no fallback
    ops.set_backend(EmuBackendEvalGrad())
    with pytest.raises(RuntimeError, match="iw_latent"):
        eng.score(x, samples=2, **kw)
    eng.close()


def test_hip_backend_validates_on_the_host():
    """HipBackend.iw_latent / iw_assemble_rows check shapes and dtypes before they touch the library, and refuse CPU tensors."""
    hip = ops.HipBackend()
    K, B, Lt = 2, 3, 8
    f32, f64 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.float64))
    mu, lv, eps, z, ratio = f32(B, Lt), f32(B, Lt), f32(K, B, Lt), f32(K, B, Lt), f64(K, B)
    for bad in ((mu[:2], lv, eps, z, ratio), (mu, lv.double(), eps, z, ratio), (mu, lv, eps[:1], z, ratio), (mu, lv, eps, z[..., :4], ratio),
                (mu, lv, eps, z, ratio.float()), (mu, lv, eps, z, f64(B, K)), (mu, f32(B, 2 * Lt)[:, :Lt], eps, z, ratio)):
        with pytest.raises(ValueError):
            hip.iw_latent(*bad, K, B, Lt)
    with pytest.raises(ValueError):
        hip.iw_latent(mu, lv, eps, z, ratio, 0, B, Lt)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.iw_latent(mu, lv, eps, z, ratio, K, B, Lt)
    bce, mse, out, ess, lw = f64(2, K, B), f64(K, B), f32(B), f32(B), f64(K, B)
    for bad in ((f64(3, K, B), mse, ratio, None, out, ess, lw), (bce.float(), mse, ratio, None, out, ess, lw),
                (bce, f64(B, K), ratio, None, out, ess, lw), (bce, mse, ratio.float(), None, out, ess, lw),
                (bce, mse, ratio, torch.ones(B, 3, dtype=torch.uint8), out, ess, lw), (bce, mse, ratio, None, f32(B + 1), ess, lw),
                (bce, mse, ratio, None, out, ess.double(), lw), (bce, mse, ratio, None, out, ess, f64(K, B + 1))):
        with pytest.raises(ValueError):
            hip.iw_assemble_rows(*bad, K, B, 1000.0)
    with pytest.raises(ValueError):
        hip.iw_assemble_rows(bce, mse, ratio, None, out, ess, lw, K, 0, 1000.0)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.iw_assemble_rows(bce, mse, ratio, None, out, ess, lw, K, B, 1000.0)


def check_problem_iw_score(device):
    """Reconstruction.iw_score: loader-format lists in, {"rows", "ess"} out; the model goes back to the mode it was in; the
    weights are re-packed on every call; a model that is no MVAE is refused."""
    inputs, targets = seeded_batch(4, 1234, with_pose=True)
    prob = SeqModeling(TM.args(no_cuda=(device == "cpu"), kl_weight=0.5), log_dir=TM.LOG_DIR, fused=False)
    prob.model.load_state_dict(seeded_state_dict(prob.model.state_dict(), 0))
    data, target = list(inputs) + [torch.ones(4, 2)], list(targets) + [torch.ones(4, 1, 64, 64)]
    prob.model.train()
    first = prob.iw_score(data, target, samples=3)
    assert prob.model.training
    assert set(first) == {"rows", "ess"} and tuple(first["rows"].shape) == (4,) and tuple(first["ess"].shape) == (4,)
    assert torch.isfinite(first["rows"]).all() and float(first["ess"].min()) >= 1.0 and float(first["ess"].max()) <= 3.0
    prob.model.eval()
    eng = prob._iw_scorer

    def same_draws_again():
        assert eng.noise.offset == 0                         # (committed: the stream position is the device counter alone)
        eng.noise.base.zero_()
    same_draws_again()
    res = prob.iw_score(data, target, samples=3)
    same_draws_again()
    again = prob.iw_score(data, target, samples=3)
    assert not prob.model.training and prob._iw_scorer is eng
    np.testing.assert_allclose(again["rows"].cpu().numpy(), res["rows"].cpu().numpy(), rtol=1e-6)
    with torch.no_grad():                                    # new weights: the next call scores the new model
        for p in prob.model.visual_decoder.parameters():
            p.mul_(0.5)
    same_draws_again()
    moved = prob.iw_score(data, target, samples=3)
    assert float((moved["rows"] - res["rows"]).abs().min()) > 0
    with pytest.raises(ValueError, match="samples"):
        prob.iw_score(data, target, samples=0)
    eng.close()
    vae = SeqModeling(TM.args(model_name="cnn-vae", input_type="visual", use_pose=False, no_cuda=(device == "cpu")),
                      log_dir=TM.LOG_DIR, fused=False)
    with pytest.raises(ValueError, match="cnn-vae"):
        vae.iw_score(data, target, samples=2)


def test_problem_iw_score():
    check_problem_iw_score("cpu")
