"""Multi-step rollout on the CPU: ``MVAEInference.rollout`` through the emulation backend (tests/emu_backend_rollout.py) against the
oracle's eval-mode forward applied to the rollout's OWN states (tests/rollout_cases.py: nothing compounds, so the tolerances are
those of one forward), against today's ``forward`` / ``complete_select`` / ``score`` called step by step, the observation
(filtering) semantics, the launch accounting, conditions, the error paths and ``DynModeling.rollout``.  The ``check_*`` functions
take the device: tests/test_rollout_gpu.py runs them on the HIP library."""
import numpy as np
import pytest
import torch

import cond_cases as CC
import rollout_cases as RC
import test_mixed_modal_emu as TMM
from emu_backend_iw import EmuBackendIW, Recorder
from emu_backend_rollout import EmuBackendRollout
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.problems.problems import DynModeling
from test_elbo_rows_emu import REL          # engine rows against the oracle: the bound that file and its GPU twin apply

OUT_TOL = TMM.OUT_TOL
T, B, L = RC.STEPS, RC.BATCH, RC.L
KW = dict(kl_weight=RC.KL_WEIGHT, pose_multiplier=RC.POSE_MULTIPLIER)
TERMS = ("bce_visual", "bce_tactile", "mse_pose", "kl", "rows")
KEYS = {"visual", "tactile", "pose", "means", "log_var"} | set(TERMS)


@pytest.fixture(autouse=True)
def emu_rollout():
    old = ops.set_backend(EmuBackendRollout())
    yield
    ops.set_backend(old)


def dev_list(ts, device):
    return None if ts is None else [None if t is None else t.to(device) for t in ts]


def keep(r):
    return {k: (None if v is None else v.detach().clone()) for k, v in r.items()}


def roll(eng, inputs, av, eps=None, **kw):
    """One rollout of the case's start; ``eps``: the T draws to inject (sample=True), None: the posterior means."""
    if eps is not None:
        eng.noise = InjectedNoise([e.clone() for e in eps], [])
    return keep(eng.rollout([inputs[0], inputs[1]], pose=inputs[2], steps=T, available=av, sample=eps is not None, **kw))


def case(device, categorical=False):
    model = TMM.build(categorical, device)
    inputs, av = RC.start()
    return model, MVAEInference(model, use_graph=False), dev_list(inputs, device), av


def states(inputs, r, device="cpu"):
    """s_0 .. s_{T-1} as [visual, tactile, pose] lists: the request, then the trajectory slots."""
    return [[t.to(device) for t in inputs]] + [[r[k][i].to(device) for k in ("visual", "tactile", "pose")] for i in range(T - 1)]


def check_one_step_consistency(device, sigmoid_atol=0.0):
    """5. Every link of the chain against the oracle's eval-mode forward of the rollout's own state s_t with the step's draw: means,
    log_var and the pose slot to OUT_TOL, the image slots against torch.sigmoid of the oracle's logits (a sigmoid divides an error
    of its argument by at least 4: OUT_TOL's atol / 4, plus ``sigmoid_atol`` for the two fp32 evaluations on the device), the
    per-step terms to REL.  The draws differ per step, so consecutive posteriors differ by far more than the tolerance: a wrong
    feedback wire cannot pass."""
    model, eng, inputs, av = case(device)
    eps, targets = RC.draws(), RC.frames(811)
    tav = RC.mixed_table(6)
    r = roll(eng, inputs, av, eps, targets=dev_list(targets, device), target_available=tav, **KW)
    assert set(r) == KEYS
    assert tuple(r["visual"].shape) == (T, B, 3, 64, 64) == tuple(r["tactile"].shape) and tuple(r["pose"].shape) == (T, B, 7)
    assert tuple(r["means"].shape) == (T, B, L) == tuple(r["log_var"].shape)
    for k in TERMS:
        assert tuple(r[k].shape) == (T, B) and r[k].dtype == (torch.float32 if k == "rows" else torch.float64), k
    for k in ("visual", "tactile"):
        assert float(r[k].min()) >= 0.0 and float(r[k].max()) <= 1.0
    prm, buf = RC.oracle_state(model)
    on0 = torch.tensor(RC.START, dtype=torch.bool)
    r = {k: v.cpu() for k, v in r.items()}
    for i, s in enumerate(states([t.cpu() for t in inputs], r)):
        v, t, pr, mu, lv = RC.oracle_step(prm, buf, s, on0 if i == 0 else None, eps[i])
        np.testing.assert_allclose(r["means"][i].numpy(), mu.numpy(), **OUT_TOL, err_msg=f"means {i}")
        np.testing.assert_allclose(r["log_var"][i].numpy(), lv.numpy(), **OUT_TOL, err_msg=f"log_var {i}")
        np.testing.assert_allclose(r["pose"][i].numpy(), pr.numpy(), **OUT_TOL, err_msg=f"pose {i}")
        for k, lg in (("visual", v), ("tactile", t)):
            d = float((r[k][i] - torch.sigmoid(lg)).abs().max())
            print("step", i, k, "largest deviation from sigmoid(oracle logits)", d)
            np.testing.assert_allclose(r[k][i].numpy(), torch.sigmoid(lg).numpy(), rtol=OUT_TOL["rtol"],
                                       atol=OUT_TOL["atol"] / 4 + sigmoid_atol, err_msg=f"{k} {i}")
        want = RC.step_terms(v, t, pr, mu, lv, [x[i] for x in targets], tav[i] != 0, RC.POSE_MULTIPLIER, RC.KL_WEIGHT)
        for k in TERMS:
            np.testing.assert_allclose(r[k][i].double().numpy(), want[k].numpy(), rtol=REL, err_msg=f"{k} {i}")
        for m, k in enumerate(TERMS[:3]):
            assert float(r[k][i][tav[i, :, m] == 0].abs().sum()) == 0.0
    moves = [float((r["means"][i + 1] - r["means"][i]).abs().median()) for i in range(T - 1)]
    print("median |means[t+1] - means[t]|", moves)
    assert min(moves) > 100 * OUT_TOL["atol"]
    eng.close()


def check_against_todays_calls(device, same=torch.equal):
    """6. The chain a caller writes today: forward() of s_t with the step's draw gives means[t] / log_var[t] bit for bit; its
    logits through complete_select(None, ...) give the trajectory slot, and score() of s_t against the step's target gives the
    step's terms -- ``same``: equal bits on the emulation, the repeatability bound of the decoders' sums on the device."""
    model, eng, inputs, av = case(device)
    eps, targets = RC.draws(), dev_list(RC.frames(812), device)
    r = roll(eng, inputs, av, eps, targets=targets, **KW)
    for i, s in enumerate(states(inputs, r, device)):
        a = av if i == 0 else None
        eng.noise = InjectedNoise([eps[i].clone()], [])
        v, t, pr, mu, lv = eng.forward([s[0], s[1]], pose=s[2], available=a)
        assert torch.equal(mu, r["means"][i]) and torch.equal(lv, r["log_var"][i]), i
        for k, (lg, logits) in zip(("visual", "tactile", "pose"), ((v, True), (t, True), (pr, False))):
            out = torch.empty_like(lg)
            ops.B.complete_select(None, lg, None, 0, out, logits)
            assert same(out, r[k][i]), (k, i, float((out - r[k][i]).abs().max()))
        eng.noise = InjectedNoise([eps[i].clone()], [])
        sc = eng.score([s[0], s[1]], pose=s[2], available=a, targets=[x[i] for x in targets], **KW)
        for k in TERMS:
            assert same(sc[k], r[k][i]), (k, i, sc[k], r[k][i])
    eng.close()


def check_observation(device, same=torch.equal):
    """7. Filtering: an all-zero table is the open loop; a fully observed modality comes back bit for bit and, with every modality
    observed, step t is forward() of the observed frame t - 1; a mixed table replaces exactly the (step, row, modality) it names."""
    model, eng, inputs, av = case(device)
    eps, obs = RC.draws(), dev_list(RC.frames(813), device)
    free = roll(eng, inputs, av, eps)
    assert all(free[k] is None for k in TERMS)
    none = roll(eng, inputs, av, eps, observed=obs, observed_available=torch.zeros(T, B, 3))
    assert torch.equal(none["means"], free["means"]) and torch.equal(none["log_var"], free["log_var"])
    assert all(same(none[k], free[k]) for k in ("visual", "tactile", "pose"))
    full = roll(eng, inputs, av, eps, observed=obs)
    assert all(torch.equal(full[k], o) for k, o in zip(("visual", "tactile", "pose"), obs))
    assert torch.equal(full["means"][0], free["means"][0])
    for i in range(1, T):
        eng.noise = InjectedNoise([eps[i].clone()], [])
        mu, lv = eng.forward([obs[0][i - 1], obs[1][i - 1]], pose=obs[2][i - 1])[3:]
        assert torch.equal(mu, full["means"][i]) and torch.equal(lv, full["log_var"][i]), i
    # touch alone keeps arriving: the other modalities stay the model's own
    touch = roll(eng, inputs, av, eps, observed=[None, obs[1], None])
    assert torch.equal(touch["tactile"], obs[1]) and same(touch["visual"][0], free["visual"][0])
    assert not torch.equal(touch["means"][1], free["means"][1])
    # a mixed table: step 0 is the open loop's step 0 except in the rows it names; every named entry holds the observation
    tab = RC.mixed_table()
    mixed = roll(eng, inputs, av, eps, observed=obs, observed_available=tab)
    for m, k in enumerate(("visual", "tactile", "pose")):
        on = (tab[:, :, m] != 0).to(device)
        assert torch.equal(mixed[k][on], obs[m][on]), k
        assert same(mixed[k][0][~on[0]], free[k][0][~on[0]]) and not torch.equal(mixed[k][~on], obs[m][~on]), k
    # [T, B, 2]: the pose is observed wherever an observed pose is given
    two = roll(eng, inputs, av, eps, observed=obs, observed_available=tab[:, :, :2])
    assert torch.equal(two["pose"], obs[2]) and torch.equal(two["visual"][0], mixed["visual"][0])
    eng.close()


def check_conditions(device):
    """11. A categorical model: a held condition [B] is the per-step condition [T, B] with equal rows; a condition that changes
    per step is forward() with that step's condition; an index out of range at step 2 is reported by bad_condition()."""
    model, eng, inputs, av = case(device, categorical=True)
    eps = RC.draws()
    held = CC.indices(B, 41).to(device)
    a = roll(eng, inputs, av, eps, condition=held)
    assert not eng.bad_condition()
    b = roll(eng, inputs, av, eps, condition=held.unsqueeze(0).repeat(T, 1))
    assert all(torch.equal(a[k], b[k]) for k in ("means", "log_var", "visual", "tactile", "pose"))
    per = torch.stack([CC.indices(B, 42 + i) for i in range(T)]).to(device)
    assert not torch.equal(per[1], per[0])
    c = roll(eng, inputs, av, eps, condition=per)
    for i, s in enumerate(states(inputs, c, device)):
        eng.noise = InjectedNoise([eps[i].clone()], [])
        mu = eng.forward([s[0], s[1]], pose=s[2], available=av if i == 0 else None, condition=per[i])[3]
        assert torch.equal(mu, c["means"][i]), i
    assert not eng.bad_condition()
    bad = per.clone()
    bad[2, 1] = CC.CAT_DIM
    roll(eng, inputs, av, eps, condition=bad)
    assert eng.bad_condition()
    roll(eng, inputs, av, eps, condition=per)
    assert not eng.bad_condition()
    with pytest.raises(ValueError):
        roll(eng, inputs, av, eps, condition=per[:2])
    with pytest.raises(ValueError):
        roll(eng, inputs, av, eps)
    eng.close()


class RecordingEngine:
    """Stands in for the problem's engine: keeps the keyword arguments of the one rollout call."""

    def __init__(self, model):
        self.model, self.calls = model, []

    def refresh(self):
        pass

    def rollout(self, x, **kw):
        self.calls.append(dict(kw, x=x))
        return {"rows": torch.zeros(1), "pose": None}


def sequences(n, l, seed=821):
    """A loader batch of n sequences of l frames, flat: (data [visual, tactile, pose, available [n*l, 2]], target [visual,
    tactile, pose, mask])."""
    from mmdyn_hip.utils.seeded_init import seeded_batch
    a, b = seeded_batch(n * l, seed, with_pose=True)
    has = torch.ones(n * l, 2, dtype=torch.float64)
    has[0] = torch.tensor([1.0, 0.0])                        # sequence 0 starts without touch
    has[1, 0], has[l + 1, 1], has[l + 2, 0] = 0.0, 0.0, 0.0  # frames that lack a modality along the way
    return a + [has], b + [torch.ones(n * l, 1, 64, 64)]


def check_problem_layer(device):
    """13. DynModeling.rollout on n = 2 sequences of l = 3 frames built by hand: what reaches the engine (a recording engine), the
    result against a direct engine call, observe=("tactile",), and the refusals."""
    n, l = 2, 3
    model = TMM.build(False, device)
    prob = TMM.problem_of(model, "cnn-mvae", False, device, DynModeling)
    prob._seq_length, prob._kl_weight, prob._pose_multiplier = l, RC.KL_WEIGHT, RC.POSE_MULTIPLIER
    data, target = sequences(n, l)
    fr = lambda t: t.reshape((n, l) + tuple(t.shape[1:]))
    rec = prob._roller = RecordingEngine(model)
    prob.rollout(data, target, observe=("tactile",))
    kw = rec.calls[0]
    assert kw["steps"] == l and kw["sample"] is False and kw["condition"] is None
    assert all(torch.equal(a.cpu(), d[::l]) for a, d in zip(kw["x"] + [kw["pose"], kw["available"]], data))
    for m in range(3):
        tg = kw["targets"][m].cpu()
        assert tuple(tg.shape[:2]) == (l, n)
        for i in range(l - 1):
            assert torch.equal(tg[i], fr(data[m])[:, i + 1]), (m, i)
        assert torch.equal(tg[l - 1], target[m][l - 1::l]), m          # the dataset's final target, the pose included
    ta = kw["target_available"].cpu()
    assert tuple(ta.shape) == (l, n, 3) and bool((ta[:, :, 2] == 1).all()) and bool((ta[l - 1] == 1).all())
    assert all(torch.equal(ta[i, :, :2], fr(data[3])[:, i + 1].to(ta.dtype)) for i in range(l - 1))
    ob, oa = kw["observed"], kw["observed_available"].cpu()
    assert ob[0] is None and ob[2] is None and torch.equal(ob[1].cpu()[:l - 1], kw["targets"][1].cpu()[:l - 1])
    assert float(oa[:, :, 0].abs().sum()) == 0.0 == float(oa[:, :, 2].abs().sum()) and float(oa[l - 1].abs().sum()) == 0.0
    assert all(torch.equal(oa[i, :, 1], fr(data[3])[:, i + 1, 1].to(oa.dtype)) for i in range(l - 1))
    prob.rollout(data, target, steps=2, observe=("visual", "pose"), sample=True)
    kw2 = rec.calls[1]
    assert kw2["steps"] == 2 and kw2["sample"] is True and tuple(kw2["targets"][0].shape[:2]) == (2, n)
    assert torch.equal(kw2["targets"][2].cpu()[1], fr(data[2])[:, 2]) and bool((kw2["observed_available"][:, :, 2] == 1).all())
    # the real engine: the result is a clone of a direct call's, and observed touch comes back where the dataset has it
    del prob._roller
    was = model.training
    res = prob.rollout(data, target, observe=("tactile",))
    assert model.training == was and set(res) == KEYS
    eng = MVAEInference(model, use_graph=False)
    want = eng.rollout(kw["x"], pose=kw["pose"], steps=l, available=kw["available"], observed=kw["observed"],
                       observed_available=kw["observed_available"], targets=kw["targets"], target_available=kw["target_available"], **KW)
    np.testing.assert_allclose(res["means"].cpu().numpy(), want["means"].cpu().numpy(), **OUT_TOL)
    np.testing.assert_allclose(res["rows"].cpu().numpy(), want["rows"].cpu().numpy(), rtol=REL)
    has = fr(data[3])[:, 1:, 1].transpose(0, 1) != 0                   # [l - 1, n]
    assert torch.equal(res["tactile"].cpu()[:l - 1][has], fr(data[1])[:, 1:].transpose(0, 1)[has])
    assert not torch.equal(res["tactile"].cpu()[:l - 1][~has], fr(data[1])[:, 1:].transpose(0, 1)[~has])
    assert float(res["bce_visual"][0, 0]) == 0.0 and float(res["bce_visual"][0, 1]) > 0.0      # frame 1 of sequence 0 lacks vision
    eng.close()
    prob._roller.close()
    for bad in (l + 1, 0, 2.0, True):
        with pytest.raises(ValueError, match="steps"):
            prob.rollout(data, target, steps=bad)
    with pytest.raises(ValueError, match="observe"):
        prob.rollout(data, target, observe=("sound",))
    with pytest.raises(ValueError):
        prob.rollout(data[0], target[0])
    vae = TMM.problem_of(model, "cnn-vae", False, device, DynModeling)
    vae._seq_length = l
    with pytest.raises(ValueError, match="cnn-vae"):
        vae.rollout(data, target)


# ---- the CPU suite ----------------------------------------------------------------------------------------------------------
def test_one_step_consistency():
    check_one_step_consistency("cpu")


def test_against_todays_calls():
    check_against_todays_calls("cpu")


def test_observation():
    check_observation("cpu")


def test_conditions():
    check_conditions("cpu")


def test_problem_layer():
    check_problem_layer("cpu")


def test_real_valued_condition_held_and_per_step():
    """A real-valued conditional model: [B, condition_dim] held is [T, B, condition_dim] with equal slices; a condition that
    changes per step changes the steps it reaches; DynModeling.rollout hands data[4] of frames 0 .. T-1 over as [T, n, cd]."""
    from mmdyn_hip.models import setup_model
    from mmdyn_hip.utils.seeded_init import seeded_running_stats, seeded_state_dict
    model = setup_model("cnn-mvae", cross_modal=True, **CC.model_kw(False, True))
    model.load_state_dict(seeded_running_stats(seeded_state_dict(model.state_dict(), 0)))
    eng = MVAEInference(model.eval(), use_graph=False)
    inputs, av = RC.start()
    held = torch.rand(B, CC.REAL_DIM, generator=torch.Generator().manual_seed(9))
    a = roll(eng, inputs, av, condition=held)
    b = roll(eng, inputs, av, condition=held.unsqueeze(0).repeat(T, 1, 1))
    assert all(torch.equal(a[k], b[k]) for k in ("means", "log_var", "visual", "tactile", "pose"))
    per = held.unsqueeze(0).repeat(T, 1, 1)
    per[1] = 1.0 - per[1]
    c = roll(eng, inputs, av, condition=per)
    assert torch.equal(c["means"][0], a["means"][0]) and not torch.equal(c["means"][1], a["means"][1])
    with pytest.raises(ValueError, match="condition"):
        roll(eng, inputs, av, condition=per[:, :2])
    eng.close()
    n, l = 2, 3
    prob = TMM.problem_of(model, "cnn-mvae", True, "cpu", DynModeling)
    prob._seq_length, prob._kl_weight, prob._pose_multiplier = l, RC.KL_WEIGHT, RC.POSE_MULTIPLIER
    data, target = sequences(n, l)
    shock = torch.rand(n * l, CC.REAL_DIM, generator=torch.Generator().manual_seed(10))
    rec = prob._roller = RecordingEngine(model)
    prob.rollout(data + [shock], target, steps=2)
    assert torch.equal(rec.calls[0]["condition"], shock.reshape(n, l, -1)[:, :2].transpose(0, 1))
    with pytest.raises(ValueError, match="shock"):
        prob.rollout(data, target)


def test_posterior_mean_rollout_draws_nothing():
    """sample=False: every step decodes its posterior mean (eps = 0) and the noise stream is not touched."""
    model, eng, inputs, av = case("cpu")
    eng.noise = InjectedNoise([], [])                                   # a draw would pop from an empty list
    mean = roll(eng, inputs, av)
    zero = roll(eng, inputs, av, [torch.zeros(B, L)] * T)
    assert all(torch.equal(mean[k], zero[k]) for k in ("means", "log_var", "visual", "tactile", "pose"))
    eng.close()


def recorded(steps, eps=True, **kw):
    model, _, inputs, av = case("cpu")
    rec = Recorder(EmuBackendRollout())
    ops.set_backend(rec)
    eng = MVAEInference(model, use_graph=False)
    runs = {}
    if eps:
        eng.noise = InjectedNoise([e for e in RC.draws(T=steps)], [])
    del rec.ops[:]
    eng.rollout([inputs[0], inputs[1]], pose=inputs[2], steps=steps, sample=eps, **kw)
    runs["rollout"] = list(rec.ops)
    for name, a in (("forward", None), ("forward_avail", RC.start()[1])):
        eng.noise = InjectedNoise(RC.draws(T=1), [])
        del rec.ops[:]
        eng.forward([inputs[0], inputs[1]], pose=inputs[2], available=a)
        runs[name] = list(rec.ops)
    eng.noise = InjectedNoise(RC.draws(T=1), [])
    del rec.ops[:]
    eng.score([inputs[0], inputs[1]], pose=inputs[2], targets=inputs)
    runs["score"] = list(rec.ops)
    eng.close()
    return runs


def test_launch_accounting():
    """8. T steps issue T x (the calls of one forward) + T feeds, in that order; step 0 takes the table, later steps do not; no
    select launch; targets add per step exactly the tail of _score; nothing else grows with T."""
    av = RC.start()[1]
    for steps in (1, 3):
        r = recorded(steps, available=av)
        fwd, fwd_av = r["forward"], r["forward_avail"]
        assert fwd_av == [("poe_fwd_avail" if o == "poe_fwd" else o) for o in fwd] and fwd.count("poe_fwd") == 1
        assert r["rollout"] == fwd_av + ["rollout_feed"] + (fwd + ["rollout_feed"]) * (steps - 1)
        assert "complete_select" not in r["rollout"] and len(fwd) > 10
        tail = r["score"][len(fwd):]
        assert tail == ["bce_logits_rows_groups", "bce_logits_rows_groups", "mse_rows_groups", "kl_rows", "elbo_assemble_rows"]
        s = recorded(steps, available=av, targets=RC.frames(814, T=steps))["rollout"]
        assert s == fwd_av + tail + ["rollout_feed"] + (fwd + tail + ["rollout_feed"]) * (steps - 1)
        s = recorded(steps, targets=RC.frames(814, T=steps), target_available=torch.ones(steps, B, 2))["rollout"]
        assert s == (fwd + tail[:-1] + ["elbo_assemble_rows_avail", "rollout_feed"]) * steps
    # the posterior-mean rollout: the same without the draw and its commit
    mean = recorded(3, eps=False, available=av)["rollout"]
    assert mean == [o for o in recorded(3, available=av)["rollout"] if o not in ("random_normal", "counter_add")]


def test_argument_errors():
    model, eng, inputs, av = case("cpu")
    x, obs = [inputs[0], inputs[1]], RC.frames(815)
    for bad in (0, -1, 2.0, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="steps"):
            eng.rollout(x, pose=inputs[2], steps=bad)
    for name in ("observed", "targets"):
        with pytest.raises(ValueError, match=name):
            eng.rollout(x, pose=inputs[2], steps=T, **{name: [t[:2] for t in obs]})
        with pytest.raises(ValueError, match=name):
            eng.rollout(x, pose=inputs[2], steps=T, **{name: [obs[0][:, :2], None, None]})
    with pytest.raises(ValueError, match="observed_available"):
        eng.rollout(x, pose=inputs[2], steps=T, observed_available=torch.ones(T, B, 3))
    with pytest.raises(ValueError, match="observed_available"):
        eng.rollout(x, pose=inputs[2], steps=T, observed=obs, observed_available=torch.ones(T - 1, B, 3))
    with pytest.raises(ValueError, match="target_available"):
        eng.rollout(x, pose=inputs[2], steps=T, targets=obs, target_available=torch.ones(B, 3))
    with pytest.raises(ValueError, match="target_available"):
        eng.rollout(x, pose=inputs[2], steps=T, target_available=torch.ones(T, B, 3))
    with pytest.raises(ValueError, match="condition"):
        eng.rollout(x, pose=inputs[2], steps=T, condition=torch.zeros(B, 3))
    with pytest.raises(ValueError, match="modality"):
        eng.rollout([None, None], steps=T)
    most = (2 ** 31 - 1) // (B * 3 * 64 * 64)
    with pytest.raises(ValueError, match=rf"largest steps for B = {B} is {most}\b"):
        eng.rollout(x, pose=inputs[2], steps=most + 1)
    eng.close()
    # a model without pose: a pose target (or observation) is refused; a backend written before the op: an error that names it
    from mmdyn_hip.models import setup_model
    import avail_cases as A
    nopose = setup_model("cnn-mvae", cross_modal=True, **dict(A.PLAIN_KW, use_pose=False)).eval()
    eng = MVAEInference(nopose, use_graph=False)
    for name in ("observed", "targets"):
        with pytest.raises(ValueError, match="pose"):
            eng.rollout(x, steps=T, **{name: obs})
    r = eng.rollout(x, steps=2, targets=[obs[0][:2], obs[1][:2], None])
    assert r["pose"] is None and r["mse_pose"] is None and tuple(r["rows"].shape) == (2, B)
    ops.set_backend(EmuBackendIW())
    with pytest.raises(RuntimeError, match="rollout_feed"):
        eng.rollout(x, steps=2)
    eng.close()


def test_hip_backend_validates_on_the_host():
    """HipBackend.rollout_feed checks shapes, dtypes, contiguity and the table before it touches the library, and refuses CPU
    tensors."""
    hip = ops.HipBackend()
    f = lambda *s: torch.zeros(*s)
    g = lambda **k: dict(dict(recon=f(B, 7), obs=f(B, 7), out=f(B, 7), logits=False, column=2), **k)
    table = torch.ones(B, 4, dtype=torch.uint8)
    for groups, tab, rows in (([], None, B), ([g()] * 5, None, B), ([g(out=f(B, 8))], None, B), ([g(obs=f(B + 1, 7))], None, B),
                              ([g(recon=f(B, 7).double())], None, B), ([g(out=f(B, 14)[:, ::2])], None, B), ([g(column=4)], None, B),
                              ([g(column=-1)], None, B), ([g()], table[:, :3], B), ([g()], table.float(), B), ([g()], table, B + 1),
                              ([g()], None, 0), ([g(recon=None)], None, B), ([g(recon=f(B, 0), obs=None, out=f(B, 0))], None, B)):
        with pytest.raises(ValueError):
            hip.rollout_feed(groups, tab, rows)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.rollout_feed([g(), g(obs=None)], table, B)


def test_emulated_feed_keeps_the_unread_side_out():
    emu, nan = EmuBackendRollout(), float("nan")
    on = torch.tensor([[1, 0, 1, 0], [0, 1, 0, 0], [1, 1, 1, 0]], dtype=torch.uint8)
    recon, obs = torch.randn(3, 5), torch.rand(3, 5)
    recon[on[:, 1] != 0], obs[on[:, 1] == 0] = nan, nan
    out = torch.full((3, 5), nan)
    emu.rollout_feed([dict(recon=recon, obs=obs, out=out, logits=True, column=1)], on, 3)
    assert torch.isfinite(out).all() and torch.equal(out[1], obs[1]) and torch.equal(out[0], torch.sigmoid(recon[0]))
