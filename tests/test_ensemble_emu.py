"""Ensemble rollout on the CPU: ``MVAEInference.rollout(sample=True, samples=N)`` through the emulation backend
(tests/emu_backend_ensemble.py).  N = 1 against today's rollout; every trajectory of N = 3 against today's rollout fed that
trajectory's slice of the draws; the statistics against an fp64 two-pass over the returned trajectories; the launch and draw
accounting; conditions; the error paths and ``DynModeling.rollout(samples=)``.  Helpers, cases and constants are those of
tests/rollout_cases.py and tests/test_rollout_emu.py (T = B = 3, 64 x 64).  The ``check_*`` functions take the device:
tests/test_ensemble_gpu.py runs them on the HIP library."""
import numpy as np
import pytest
import torch

import cond_cases as CC
import rollout_cases as RC
import test_mixed_modal_emu as TMM
import test_rollout_emu as E
from emu_backend_ensemble import EmuBackendEnsemble
from emu_backend_iw import Recorder
from emu_backend_rollout import EmuBackendRollout
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.problems.problems import DynModeling
from test_elbo_rows_gpu import RTOL_SUM          # (that file's constant, not a new one)

OUT_TOL, REL = E.OUT_TOL, E.REL
T, B, L = E.T, E.B, E.L
N = 3
KW = E.KW
STATES = ("visual", "tactile", "pose")
STATS = tuple(f"{m}_{s}" for m in STATES for s in ("mean", "var"))
KEYS = E.KEYS | set(STATS) | {"spread"}
# the bounds of the statistics: one fp32 rounding plus the fp64 error of the single pass, times 2 (mean) and 4 (variance)
MEAN_ULP, VAR_REL, VAR_ABS = 2.0 ** -23, 2.0 ** -22, 2.0 ** -126


@pytest.fixture(autouse=True)
def emu_ensemble():
    old = ops.set_backend(EmuBackendEnsemble())
    yield
    ops.set_backend(old)


def blocks(n, seed=34):
    """T distinct standard-normal draws [n * B, L]: what step t of an ensemble of n asks for."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n * B, L, generator=g) for _ in range(T)]


def eroll(eng, inputs, av, eps, n, **kw):
    """One ensemble rollout of the case's start with the T blocks ``eps`` injected."""
    eng.noise = InjectedNoise([e.clone() for e in eps], [])
    return E.keep(eng.rollout([inputs[0], inputs[1]], pose=inputs[2], steps=T, available=av, sample=True, samples=n, **kw))


def check_shapes(r, n):
    assert set(r) == KEYS
    assert tuple(r["visual"].shape) == (T, n, B, 3, 64, 64) == tuple(r["tactile"].shape) and tuple(r["pose"].shape) == (T, n, B, 7)
    for m in STATES:
        assert tuple(r[m + "_mean"].shape) == tuple(r[m + "_var"].shape) == (T, B) + tuple(r[m].shape[3:]), m
    assert tuple(r["spread"].shape) == (T, 3, B) and r["spread"].dtype == torch.float64
    assert tuple(r["means"].shape) == (T, n, B, L) == tuple(r["log_var"].shape)


def check_one_sample_is_todays_rollout(device, same=torch.equal):
    """1. samples=1 against rollout(sample=True) with the same draws, targets, observations and mixed tables: every shared key
    equal bit for bit with the N axis squeezed -- same shapes, same routes (``same``: what the terms, which fp64 atomics add on the
    device, are compared with); the mean is the prediction BEFORE the observation
    (the state wherever nothing was taken, and step 0 of the open loop everywhere), the variance and the spread are 0."""
    model, eng, inputs, av = E.case(device)
    eps = RC.draws()
    obs, tgs = E.dev_list(RC.frames(871), device), E.dev_list(RC.frames(872), device)
    otab, ttab = RC.mixed_table(9), RC.mixed_table(10)
    kw = dict(observed=obs, observed_available=otab, targets=tgs, target_available=ttab, **KW)
    a = eroll(eng, inputs, av, eps, 1, **kw)
    b = E.roll(eng, inputs, av, eps, **kw)
    check_shapes(a, 1)
    for k in E.KEYS:
        assert a[k].shape[1] == 1 and a[k].dtype == b[k].dtype, k
        eq = same if k in E.TERMS else torch.equal
        assert eq(a[k][:, 0], b[k]), (k, float((a[k][:, 0].double() - b[k].double()).abs().max()))
    free = E.roll(eng, inputs, av, eps)
    for m, k in enumerate(STATES):
        on = (otab[:, :, m] != 0).to(device)
        assert torch.equal(a[k][:, 0][on], obs[m][on]), k
        assert torch.equal(a[k + "_mean"][~on], a[k][:, 0][~on]), k
        assert torch.equal(a[k + "_mean"][0], free[k][0]), k
        assert float(a[k + "_var"].abs().max()) == 0.0, k
    assert float(a["spread"].abs().max()) == 0.0
    eng.close()


def check_every_trajectory(device):
    """2. N = 3 with mixed observations (touch never observed) and targets: trajectory n is today's rollout fed slice n of every
    step's draw -- states and posteriors to OUT_TOL (the image slots: a sigmoid divides an error of its argument by at least 4, so
    OUT_TOL holds a fortiori), terms to REL; a row that takes an observation holds it bit for bit in all N trajectories."""
    model, eng, inputs, av = E.case(device)
    eps = blocks(N)
    obs, tgs = E.dev_list(RC.frames(873), device), E.dev_list(RC.frames(874), device)
    otab, ttab = RC.mixed_table(11), RC.mixed_table(12)
    assert bool((otab[:, :, 0] != 0).any()) and bool((otab[:, :, 0] == 0).any())
    kw = dict(observed=[obs[0], None, obs[2]], observed_available=otab, targets=tgs, target_available=ttab, **KW)
    e = eroll(eng, inputs, av, eps, N, **kw)
    check_shapes(e, N)
    for n in range(N):
        r = E.roll(eng, inputs, av, [x.view(N, B, L)[n] for x in eps], **kw)
        for k in ("means", "log_var") + STATES:
            np.testing.assert_allclose(e[k][:, n].cpu().numpy(), r[k].cpu().numpy(), **OUT_TOL, err_msg=f"{k} trajectory {n}")
        for k in E.TERMS:
            np.testing.assert_allclose(e[k][:, n].double().cpu().numpy(), r[k].double().cpu().numpy(), rtol=REL, err_msg=f"{k} {n}")
        for m in (0, 2):
            on = (otab[:, :, m] != 0).to(device)
            assert torch.equal(e[STATES[m]][:, n][on], obs[m][on]), (m, n)
        assert not torch.equal(e["tactile"][:, n], obs[1])
    assert torch.equal(e["means"][0, 0], e["means"][0, 1]) and torch.equal(e["means"][0, 0], e["means"][0, N - 1])
    assert not torch.equal(e["means"][1, 0], e["means"][1, 1])             # the trajectories part at the first draw
    eng.close()


def stats_ref(p):
    """fp64 two-pass mean and population variance over axis 0 of p [N, ...], and max_n |p_n|."""
    p = p.double()
    m = p.mean(0)
    return m, ((p - m) ** 2).mean(0), p.abs().amax(0)


def assert_stats(mean, var, spread, p, what=""):
    """mean / var [B, ...] and spread [B] (None: not checked) against the two-pass reference over p [N, B, ...]."""
    m, v, top = stats_ref(p)
    dm, dv = (mean.double() - m).abs(), (var.double() - v).abs()
    print(what, "mean: largest error in units of 2^-23 max|p|", float((dm / (MEAN_ULP * top).clamp_min(1e-300)).max()),
          "var: largest error / bound", float((dv / (VAR_REL * v + VAR_ABS)).max()))
    assert bool((dm <= MEAN_ULP * top).all()), what
    assert bool((dv <= VAR_REL * v + VAR_ABS).all()), what
    if spread is not None:
        want = var.double().reshape(var.shape[0], -1).sum(1)
        assert torch.allclose(spread, want, rtol=RTOL_SUM, atol=0.0), (what, spread, want)


def check_statistics(device):
    """3. Nothing observed, so the returned trajectories ARE the predictions: the mean, the variance and the spread of every step
    and modality against an fp64 two-pass over them."""
    model, eng, inputs, av = E.case(device)
    e = eroll(eng, inputs, av, blocks(N, 35), N)
    assert all(e[k] is None for k in E.TERMS)
    for m, k in enumerate(STATES):
        for i in range(T):
            assert_stats(e[k + "_mean"][i].cpu(), e[k + "_var"][i].cpu(), e["spread"][i, m].cpu(), e[k][i].cpu(), f"{k} step {i}")
        assert float(e[k + "_var"][1:].max()) > 0.0
    eng.close()


def check_conditions(device):
    """6. A categorical model: a held condition [B] and the same condition per step [T, B] give equal results; trajectory n under a
    per-step condition is today's rollout with that condition and slice n of the draws (the condition of row b reaches row
    n * B + b); an index out of range at step 2 is reported by bad_condition()."""
    model, eng, inputs, av = E.case(device, categorical=True)
    eps = blocks(2, 36)
    held = CC.indices(B, 43).to(device)
    a = eroll(eng, inputs, av, eps, 2, condition=held)
    assert not eng.bad_condition()
    b = eroll(eng, inputs, av, eps, 2, condition=held.unsqueeze(0).repeat(T, 1))
    assert all(torch.equal(a[k], b[k]) for k in ("means", "log_var") + STATES)
    per = torch.stack([CC.indices(B, 44 + i) for i in range(T)]).to(device)
    c = eroll(eng, inputs, av, eps, 2, condition=per)
    for n in range(2):
        r = E.roll(eng, inputs, av, [x.view(2, B, L)[n] for x in eps], condition=per)
        for k in ("means", "log_var", "pose"):
            np.testing.assert_allclose(c[k][:, n].cpu().numpy(), r[k].cpu().numpy(), **OUT_TOL, err_msg=f"{k} trajectory {n}")
    assert not eng.bad_condition()
    bad = per.clone()
    bad[2, 1] = CC.CAT_DIM
    eroll(eng, inputs, av, eps, 2, condition=bad)
    assert eng.bad_condition()
    eroll(eng, inputs, av, eps, 2, condition=per)
    assert not eng.bad_condition()
    eng.close()


# ---- the CPU suite ----------------------------------------------------------------------------------------------------------
def test_one_sample_is_todays_rollout():
    check_one_sample_is_todays_rollout("cpu")


def test_every_trajectory_is_todays_rollout_on_its_draws():
    check_every_trajectory("cpu")


def test_statistics():
    check_statistics("cpu")


def test_conditions():
    check_conditions("cpu")


def test_real_valued_condition_reaches_every_trajectory():
    """6. A real-valued conditional model: held [B, cd] is per-step [T, B, cd] with equal slices, and trajectory n is today's rollout
    with the same condition on slice n of the draws."""
    from mmdyn_hip.models import setup_model
    from mmdyn_hip.utils.seeded_init import seeded_running_stats, seeded_state_dict
    model = setup_model("cnn-mvae", cross_modal=True, **CC.model_kw(False, True))
    model.load_state_dict(seeded_running_stats(seeded_state_dict(model.state_dict(), 0)))
    eng = MVAEInference(model.eval(), use_graph=False)
    inputs, av = RC.start()
    eps = blocks(2, 37)
    held = torch.rand(B, CC.REAL_DIM, generator=torch.Generator().manual_seed(11))
    a = eroll(eng, inputs, av, eps, 2, condition=held)
    b = eroll(eng, inputs, av, eps, 2, condition=held.unsqueeze(0).repeat(T, 1, 1))
    assert all(torch.equal(a[k], b[k]) for k in ("means", "log_var") + STATES)
    for n in range(2):
        r = E.roll(eng, inputs, av, [x.view(2, B, L)[n] for x in eps], condition=held)
        np.testing.assert_allclose(a["means"][:, n].numpy(), r["means"].numpy(), **OUT_TOL, err_msg=f"trajectory {n}")
    eng.close()


class ShapeRecorder(Recorder):
    """A Recorder that also keeps, per call, the shapes of every tensor the call was handed (``sigs``)."""

    def __init__(self, inner):
        super().__init__(inner)
        object.__setattr__(self, "sigs", [])

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name.startswith("_") or not callable(getattr(self.inner, name)):
            return call

        def shaped(*a, **k):
            self.sigs.append((name, tuple(tuple(t.shape) for t in _tensors_of((a, k)))))
            return call(*a, **k)
        return shaped


def _tensors_of(a):
    if torch.is_tensor(a):
        return [a]
    if isinstance(a, (list, tuple)):
        return [t for x in a for t in _tensors_of(x)]
    if isinstance(a, dict):
        return [t for x in a.values() for t in _tensors_of(x)]
    return []


def test_launch_accounting():
    """4. The calls of an ensemble rollout, by name and by the shapes they are handed.  With F(rows) the calls of today's
    forward() on that many rows (the PoE launch at index p): step 0 = F(B)[:p] (the trunks and heads see B rows), the PoE launch
    on the table, ONE iw_latent, F(N B)[p + 1:] (the decoders see N * B rows); every later step = F(N B); each step ends in one
    ensemble_feed; no rollout_feed, no complete_select.  With targets a step adds the row kernels (one launch per term up to
    ROW_GROUPS_MAX trajectories), kl_rows and the assembly.  samples=None records today's list."""
    model, _, inputs, av = E.case("cpu")
    rec = ShapeRecorder(EmuBackendEnsemble())
    ops.set_backend(rec)
    eng = MVAEInference(model, use_graph=False)
    x, pose = [inputs[0], inputs[1]], inputs[2]

    def run(fn):
        del rec.ops[:], rec.sigs[:]
        fn()
        return list(rec.ops), list(rec.sigs)

    def fwd(n):
        eng.noise = InjectedNoise([torch.zeros(n * B, L)], [])
        rp = lambda t: t.repeat((n,) + (1,) * (t.dim() - 1))
        return run(lambda: eng.forward([rp(x[0]), rp(x[1])], pose=rp(pose)))
    (fb, sb), (fnb, snb) = fwd(1), fwd(N)
    assert fb == fnb and fb.count("poe_fwd") == 1 and len(fb) > 10
    p = fb.index("poe_fwd")

    def ens(**kw):
        eng.noise = InjectedNoise(blocks(N), [])
        return run(lambda: eng.rollout(x, pose=pose, steps=T, available=av, sample=True, samples=N, **kw))
    names, sigs = ens()
    step0 = fb[:p] + ["poe_fwd_avail", "iw_latent"] + fb[p + 1:]
    assert names == step0 + ["ensemble_feed"] + (fb + ["ensemble_feed"]) * (T - 1)
    assert names.count("iw_latent") == 1 and names.count("ensemble_feed") == T
    assert "rollout_feed" not in names and "complete_select" not in names
    assert sigs[:p] == sb[:p]                                                   # step 0's trunks and heads: B rows
    assert sigs[p + 2:len(step0)] == snb[p + 1:]                                # its decoders: N * B rows
    for i in range(1, T):                                                       # every later launch: N * B rows
        lo = (len(step0) + 1) + (i - 1) * (len(fb) + 1)
        assert sigs[lo:lo + len(fb)] == snb, i
    assert sb != snb
    tail = ["bce_logits_rows_groups", "bce_logits_rows_groups", "mse_rows_groups", "kl_rows", "elbo_assemble_rows"]
    names, _ = ens(targets=RC.frames(875))
    assert names == step0 + tail + ["ensemble_feed"] + (fb + tail + ["ensemble_feed"]) * (T - 1)
    names, _ = ens(targets=RC.frames(875), target_available=torch.ones(T, B, 2))
    assert names.count("elbo_assemble_rows_avail") == T and names.count("elbo_assemble_rows") == 0
    # samples=None: today's path on a backend that lacks the new op
    ops.set_backend(Recorder(EmuBackendRollout()))
    today = E.recorded(T, available=av)["rollout"]
    rec2 = Recorder(EmuBackendEnsemble())
    ops.set_backend(rec2)
    eng2 = MVAEInference(model, use_graph=False)
    eng2.noise = InjectedNoise(RC.draws(), [])
    del rec2.ops[:]                                                            # (the constructor packed the weights)
    eng2.rollout(x, pose=pose, steps=T, available=av, sample=True)
    assert rec2.ops == today and "ensemble_feed" not in today
    eng.close(), eng2.close()


class CountingNoise:
    """A noise source that lists the shapes it is asked for."""

    def __init__(self, seed=0):
        self.asked, self.commits, self.g = [], 0, torch.Generator().manual_seed(seed)

    def eps(self, shape, device):
        self.asked.append(tuple(shape))
        return torch.randn(*shape, generator=self.g).to(device)

    def keep_mask(self, shape, device):
        raise AssertionError("an eval-mode rollout draws no dropout mask")

    def commit(self):
        self.commits += 1


def test_draw_accounting():
    """5. The draws requested from the noise source: T blocks of N * B * L normals, (N * B, L) or (N, B, L), and nothing else."""
    model, eng, inputs, av = E.case("cpu")
    for n in (1, N):
        eng.noise = noise = CountingNoise()
        eng.rollout([inputs[0], inputs[1]], pose=inputs[2], steps=T, available=av, sample=True, samples=n, targets=RC.frames(876))
        assert len(noise.asked) == T and noise.commits == T
        assert noise.asked[0] in ((n * B, L), (n, B, L)) and noise.asked[1:] == [(n * B, L)] * (T - 1)
    eng.close()


def test_argument_errors():
    """7."""
    model, eng, inputs, av = E.case("cpu")
    x = [inputs[0], inputs[1]]
    for bad in (0, -1, True, 2.5, "2"):
        with pytest.raises(ValueError, match="samples"):
            eng.rollout(x, pose=inputs[2], steps=T, sample=True, samples=bad)
    with pytest.raises(ValueError, match="N identical trajectories"):
        eng.rollout(x, pose=inputs[2], steps=T, samples=2)
    most = min((2 ** 31 - 1) // (T * B * 3 * 64 * 64), (2 ** 31 - 1) // (B * 32 * 32 * 32))
    with pytest.raises(ValueError, match=rf"largest samples for B = {B} and steps = {T} is {most}\b"):
        eng.rollout(x, pose=inputs[2], steps=T, sample=True, samples=most + 1)
    one = min((2 ** 31 - 1) // (B * 3 * 64 * 64), (2 ** 31 - 1) // (B * 32 * 32 * 32))
    assert one < (2 ** 31 - 1) // (B * 3 * 64 * 64)                             # one step: the decoder activation binds first
    with pytest.raises(ValueError, match=rf"largest samples for B = {B} and steps = 1 is {one}\b"):
        eng.rollout(x, pose=inputs[2], steps=1, sample=True, samples=one + 1)
    eng.close()
    # a model without pose: the pose entries are None and the pose row of spread stays 0
    from mmdyn_hip.models import setup_model
    import avail_cases as A
    nopose = setup_model("cnn-mvae", cross_modal=True, **dict(A.PLAIN_KW, use_pose=False)).eval()
    eng = MVAEInference(nopose, use_graph=False)
    obs = RC.frames(877)
    eng.noise = InjectedNoise(blocks(2)[:2], [])
    r = eng.rollout(x, steps=2, sample=True, samples=2, targets=[obs[0][:2], obs[1][:2], None])
    assert r["pose"] is None and r["pose_mean"] is None and r["pose_var"] is None and r["mse_pose"] is None
    assert tuple(r["rows"].shape) == (2, 2, B) and float(r["spread"][:, 2].abs().max()) == 0.0 and float(r["spread"][:, :2].min()) > 0.0
    # a backend written before the op: an error that names it
    ops.set_backend(EmuBackendRollout())
    with pytest.raises(RuntimeError, match="ensemble_feed"):
        eng.rollout(x, steps=2, sample=True, samples=2)
    eng.close()


def test_hip_backend_validates_on_the_host():
    """HipBackend.ensemble_feed checks shapes, dtypes, contiguity and the table before it touches the library, and refuses CPU
    tensors."""
    hip, n = ops.HipBackend(), 2
    f = lambda *s: torch.zeros(*s)
    g = lambda **k: dict(dict(recon=f(n * B, 7), obs=f(B, 7), out=f(n * B, 7), mean=f(B, 7), var=f(B, 7),
                              spread=torch.zeros(B, dtype=torch.float64), logits=False, column=2), **k)
    table = torch.ones(B, 4, dtype=torch.uint8)
    for groups, tab, nn, rows in (([], None, n, B), ([g()] * 5, None, n, B), ([g(out=f(n * B, 8))], None, n, B),
                                  ([g(out=f(B, 7))], None, n, B), ([g(obs=f(n * B, 7))], None, n, B), ([g(mean=f(B, 8))], None, n, B),
                                  ([g(var=f(B + 1, 7))], None, n, B), ([g(recon=f(n * B, 7).double())], None, n, B),
                                  ([g(mean=f(B, 14)[:, ::2])], None, n, B), ([g(spread=torch.zeros(B))], None, n, B),
                                  ([g(spread=torch.zeros(B + 1, dtype=torch.float64))], None, n, B), ([g(var=None)], None, n, B),
                                  ([g(column=4)], None, n, B), ([g(column=-1)], None, n, B), ([g()], table[:, :3], n, B),
                                  ([g()], table.float(), n, B), ([g()], table, n, B + 1), ([g()], None, 0, B), ([g()], None, n, 0),
                                  ([g(mean=None)], None, n, B),
                                  ([g(recon=f(n * B, 0), obs=None, out=f(n * B, 0), mean=f(B, 0), var=f(B, 0))], None, n, B)):
        with pytest.raises(ValueError):
            hip.ensemble_feed(groups, tab, nn, rows)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.ensemble_feed([g(), g(obs=None, var=None, spread=None)], table, n, B)


def test_emulated_feed_keeps_the_unread_side_out_and_counts_every_row():
    emu, nan = EmuBackendEnsemble(), float("nan")
    on = torch.tensor([[1, 0, 1, 0], [0, 1, 0, 0], [1, 1, 1, 0]], dtype=torch.uint8)
    recon, obs = torch.randn(2 * 3, 5), torch.rand(3, 5)
    obs[on[:, 1] == 0] = nan
    out, mean, var = torch.full((6, 5), nan), torch.full((3, 5), nan), torch.full((3, 5), nan)
    spread = torch.zeros(3, dtype=torch.float64)
    emu.ensemble_feed([dict(recon=recon, obs=obs, out=out, mean=mean, var=var, spread=spread, logits=True, column=1)], on, 2, 3)
    assert torch.isfinite(out).all() and torch.equal(out[1], obs[1]) and torch.equal(out[4], obs[1])
    assert torch.equal(out[0], torch.sigmoid(recon[0])) and torch.equal(out[3], torch.sigmoid(recon[3]))
    assert_stats(mean, var, spread, torch.sigmoid(recon).view(2, 3, 5))        # the observed row's statistics too


def test_problem_layer():
    """8. DynModeling.rollout(samples=2): the argument reaches the engine, the new keys come back with their shapes, and the model
    goes back to its mode."""
    n, l = 2, 3
    model = TMM.build(False, "cpu")
    prob = TMM.problem_of(model, "cnn-mvae", False, "cpu", DynModeling)
    prob._seq_length, prob._kl_weight, prob._pose_multiplier = l, RC.KL_WEIGHT, RC.POSE_MULTIPLIER
    data, target = E.sequences(n, l)
    rec = prob._roller = E.RecordingEngine(model)
    prob.rollout(data, target, sample=True, samples=2)
    prob.rollout(data, target, sample=True)
    assert rec.calls[0]["samples"] == 2 and rec.calls[0]["sample"] is True and "samples" not in rec.calls[1]
    del prob._roller
    model.train()
    res = prob.rollout(data, target, observe=("tactile",), sample=True, samples=2)
    assert model.training and set(res) == KEYS
    assert tuple(res["visual"].shape) == (l, 2, n, 3, 64, 64) and tuple(res["pose"].shape) == (l, 2, n, 7)
    assert tuple(res["tactile_var"].shape) == (l, n, 3, 64, 64) and tuple(res["pose_mean"].shape) == (l, n, 7)
    assert tuple(res["spread"].shape) == (l, 3, n) and tuple(res["rows"].shape) == (l, 2, n) == tuple(res["kl"].shape)
    assert float(res["spread"][:, :2].min()) > 0.0
    prob._roller.close()
    with pytest.raises(ValueError, match="samples"):
        prob.rollout(data, target, sample=True, samples=0)
    with pytest.raises(ValueError, match="N identical trajectories"):
        prob.rollout(data, target, samples=2)
