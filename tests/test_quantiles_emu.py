"""Ensemble quantiles on the CPU: ``MVAEInference.rollout(sample=True, samples=N, quantiles=...)`` through the emulation backend
(tests/emu_backend_quantiles.py) against the restatement of tests/quantile_cases.py (a sort and single fp64 operations) applied
to the returned trajectories; the prediction quantiles under observations; ``rows_q``; order and bounds; the textbook definition;
the launch accounting and the graph key; the error paths and ``DynModeling.rollout(samples=, quantiles=)``.  Helpers, cases and
constants are those of tests/test_ensemble_emu.py and tests/rollout_cases.py (T = B = 3, N = 3, 64 x 64).  The ``check_*`` functions
take the device: tests/test_quantiles_gpu.py runs them on the HIP library."""
import pytest
import torch

import quantile_cases as QC
import rollout_cases as RC
import test_ensemble_emu as EE
import test_mixed_modal_emu as TMM
import test_rollout_emu as E
from emu_backend_ensemble import EmuBackendEnsemble
from emu_backend_quantiles import EmuBackendQuantiles
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.problems.problems import DynModeling

T, B, L, N = EE.T, EE.B, EE.L, EE.N
KW = EE.KW
STATES = EE.STATES
QS = (0.0, 0.25, 0.5, 1.0)              # at N = 3: h = 0, 0.5, 1, 2 -- three exact order statistics and one interpolated
QKEYS = ("visual_q", "tactile_q", "pose_q", "rows_q")
KEYS = EE.KEYS | set(QKEYS)


@pytest.fixture(autouse=True)
def emu_quantiles():
    old = ops.set_backend(EmuBackendQuantiles())
    yield
    ops.set_backend(old)


def qroll(eng, inputs, av, eps, n, quantiles=QS, **kw):
    return EE.eroll(eng, inputs, av, eps, n, quantiles=quantiles, **kw)


def restated(traj, quantiles, n):
    """The restatement on every step of traj [T, n, B, ...] -> [T, Q, B, ...]."""
    lo, frac = QC.index_of(quantiles, n)
    return torch.stack([QC.restate(traj[i], lo, frac) for i in range(traj.shape[0])])


def check_shapes(device):
    """1. Shapes, dtypes and the key set: the ensemble's keys plus the four new ones; rows_q None without targets, pose_q None
    without a pose model; without ``quantiles`` the ensemble's key set, unchanged."""
    model, eng, inputs, av = E.case(device)
    tgs = E.dev_list(RC.frames(901), device)
    r = qroll(eng, inputs, av, EE.blocks(N), N, targets=tgs, **KW)
    assert set(r) == KEYS
    Q = len(QS)
    for k in ("visual_q", "tactile_q"):
        assert tuple(r[k].shape) == (T, Q, B, 3, 64, 64) and r[k].dtype == torch.float32, k
    assert tuple(r["pose_q"].shape) == (T, Q, B, 7) and r["pose_q"].dtype == torch.float32
    assert tuple(r["rows_q"].shape) == (T, Q, B) and r["rows_q"].dtype == torch.float32
    assert tuple(r["rows"].shape) == (T, N, B) and tuple(r["visual"].shape) == (T, N, B, 3, 64, 64)
    r = qroll(eng, inputs, av, EE.blocks(N), N, quantiles=[0.5])
    assert set(r) == KEYS and r["rows_q"] is None and r["rows"] is None and tuple(r["pose_q"].shape) == (T, 1, B, 7)
    assert set(EE.eroll(eng, inputs, av, EE.blocks(N), N)) == EE.KEYS
    eng.close()
    from mmdyn_hip.models import setup_model
    import avail_cases as A
    nopose = setup_model("cnn-mvae", cross_modal=True, **dict(A.PLAIN_KW, use_pose=False)).to(device).eval()
    eng = MVAEInference(nopose, use_graph=False)
    eng.noise = InjectedNoise(EE.blocks(2)[:2], [])
    r = eng.rollout([inputs[0], inputs[1]], steps=2, sample=True, samples=2, quantiles=(0.1, 0.9),
                    targets=[tgs[0][:2], tgs[1][:2], None])
    assert set(r) == KEYS and r["pose_q"] is None and r["pose"] is None
    assert tuple(r["visual_q"].shape) == (2, 2, B, 3, 64, 64) and tuple(r["rows_q"].shape) == (2, 2, B)
    eng.close()


def check_open_loop(device):
    """2. Nothing observed, so the state IS the prediction: ``*_q`` has the bits of the restatement on the returned trajectories;
    q = 0 is the minimum and q = 1 the maximum over n, q = 0.5 at N = 3 an element of the trajectory (numerically, ``==``).
    6. Against numpy.quantile of the fp64-widened samples: within 2^-23 max(|s_lo|, |s_hi|) per element -- the kernel's value is one
    fp32 rounding of an fp64 evaluation whose own error is far below that."""
    model, eng, inputs, av = E.case(device)
    r = qroll(eng, inputs, av, EE.blocks(N, 41), N)
    lo, _ = QC.index_of(QS, N)
    for k in STATES:
        traj, got = r[k], r[k + "_q"]
        assert not bool(torch.isnan(got).any()), k
        d = QC.first_diff(got, restated(traj, QS, N))
        assert d is None, (k, d)
        assert bool((got[:, 0] == traj.amin(1)).all()) and bool((got[:, 3] == traj.amax(1)).all()), k
        assert bool((got[:, 2].unsqueeze(1) == traj).any(1).all()), k
        assert not torch.equal(got[:, 0], got[:, 3]), k
        for i in range(T):
            s_lo, s_hi = QC.neighbours(traj[i], lo)
            bound = 2.0 ** -23 * torch.maximum(s_lo.abs(), s_hi.abs()).double().cpu()
            err = (got[i].double().cpu() - QC.textbook(traj[i], QS)).abs()
            print(k, "step", i, "largest error against numpy.quantile in units of the bound",
                  float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (k, i)
    eng.close()


def check_under_observations(device):
    """3. A mixed table with touch observed: the quantiles describe the PREDICTION.  Step 0 does not depend on what is observed
    afterwards: ``*_q[0]`` equals the open loop's on every row; where a (step, row) takes no observation the kept trajectory is the
    prediction and the restatement on it has the bits of ``*_q``; on an observed row ``*_q`` is not the observation."""
    model, eng, inputs, av = E.case(device)
    eps = EE.blocks(N, 42)
    obs, otab = E.dev_list(RC.frames(902), device), RC.mixed_table(15)
    on = (otab[:, :, 1] != 0).to(device)
    assert bool(on.any()) and bool((~on).any()) and bool(on[0].any())
    r = qroll(eng, inputs, av, eps, N, observed=[None, obs[1], None], observed_available=otab)
    free = qroll(eng, inputs, av, eps, N)
    for k in STATES:
        assert torch.equal(r[k + "_q"][0], free[k + "_q"][0]), k
    for k in ("visual", "pose"):
        d = QC.first_diff(r[k + "_q"], restated(r[k], QS, N))
        assert d is None, (k, d)
    want, got = restated(r["tactile"], QS, N), r["tactile_q"]
    assert torch.equal(r["tactile"][:, 0][on], obs[1][on])                   # the kept trajectory holds the observation there
    for i in range(T):
        d = QC.first_diff(got[i][:, ~on[i]], want[i][:, ~on[i]])
        assert d is None, (i, d)
        for b in range(B):
            if bool(on[i, b]):
                for j in range(len(QS)):
                    assert not torch.equal(got[i, j, b], obs[1][i, b]), (i, j, b)
                assert not torch.equal(got[i, 0, b], got[i, 3, b]), (i, b)   # N equal samples would give equal quantiles
    eng.close()


def check_rows(device, exact=True):
    """4. ``rows_q`` against the restatement on the returned ``rows``: the bits on the emulation; on the device ``exact=False``
    compares within RTOL_SUM x max |rows| of the (step, row) column -- an order statistic moves by at most its samples' largest
    move, and ``rows`` comes from fp64 atomics."""
    model, eng, inputs, av = E.case(device)
    tgs, ttab = E.dev_list(RC.frames(903), device), RC.mixed_table(16)
    r = qroll(eng, inputs, av, EE.blocks(N, 43), N, targets=tgs, target_available=ttab, **KW)
    want = restated(r["rows"], QS, N)
    if exact:
        assert QC.first_diff(r["rows_q"], want) is None
    else:
        bound = EE.RTOL_SUM * r["rows"].abs().amax(1, keepdim=True)
        assert bool(((r["rows_q"] - want).abs() <= bound).all())
    assert bool((r["rows_q"][:, 0] == r["rows"].amin(1)).all()) and bool((r["rows_q"][:, 3] == r["rows"].amax(1)).all())
    assert not torch.equal(r["rows_q"][:, 0], r["rows_q"][:, 3])
    eng.close()


def check_order_and_bounds(device):
    """5. Ascending q give non-decreasing results inside [s_lo, s_hi]; samples=1 gives every quantile equal to the prediction and
    rows_q equal to rows; N identical trajectories give identical quantiles."""
    model, eng, inputs, av = E.case(device)
    tgs = E.dev_list(RC.frames(904), device)
    qs = (0.0, 0.1, 0.25, 0.5, 0.5, 0.8, 1.0)
    r = qroll(eng, inputs, av, EE.blocks(N, 44), N, quantiles=qs, targets=tgs, **KW)
    lo, _ = QC.index_of(qs, N)
    for k, src in zip(STATES + ("rows",), STATES + ("rows",)):
        got = r[k + "_q"]
        assert bool((got[:, 1:] >= got[:, :-1]).all()), k
        assert torch.equal(got[:, 3], got[:, 4]), k
        for i in range(T):
            s_lo, s_hi = QC.neighbours(r[src][i], lo)
            assert bool(((s_lo <= got[i]) & (got[i] <= s_hi)).all()), (k, i)
    one = qroll(eng, inputs, av, RC.draws(), 1, quantiles=qs, targets=tgs, **KW)
    for k in STATES + ("rows",):
        for j in range(len(qs)):
            assert torch.equal(one[k + "_q"][:, j], one[k][:, 0]), (k, j)
    same = [e.repeat(N, 1) for e in RC.draws(45)]                            # the N slices of every step's draw are one draw
    r = qroll(eng, inputs, av, same, N, quantiles=qs)
    for k in STATES:
        # (a GEMM over N * B rows need not round row n * B + b as it rounds row b: the elements that did come out identical)
        alike = (r[k] == r[k][:, :1]).all(1)
        print(k, "elements with N identical samples:", int(alike.sum()), "of", alike.numel())
        assert int(alike.sum()) >= alike[0].numel() // 2, k                  # (step 0 decodes N copies of one latent)
        for j in range(len(qs)):
            assert torch.equal(r[k + "_q"][:, j][alike], r[k][:, 0][alike]), (k, j)
    eng.close()


# ---- the CPU suite ----------------------------------------------------------------------------------------------------------
def test_shapes_dtypes_and_keys():
    check_shapes("cpu")


def test_open_loop_quantiles_are_the_restatement_on_the_trajectories():
    check_open_loop("cpu")


def test_quantiles_describe_the_prediction_under_observations():
    check_under_observations("cpu")


def test_rows_quantiles():
    check_rows("cpu")


def test_order_and_bounds():
    check_order_and_bounds("cpu")


def test_host_index_of_a_quantile():
    """The engine's (lo, frac) against the restatement of tests/quantile_cases.py, and the corner q = 1."""
    for n in (1, 2, 3, 8, 9, 64, 127, 128):
        qs = (0.0, 1.0, 0.5, 0.05, 0.95, 1.0 / 3.0, 0.999999, 0.25)
        assert MVAEInference._quantile_index(qs, n) == QC.index_of(qs, n), n
        lo, frac = MVAEInference._quantile_index((1.0, 0.0), n)
        assert lo == [n - 1, 0] and frac == [0.0, 0.0]
    assert MVAEInference._quantile_index(QS, 3) == ([0, 0, 1, 2], [0.0, 0.5, 0.0, 0.0])


def test_launch_accounting():
    """7. With ``quantiles``: the calls of the ensemble rollout plus exactly one ensemble_quantiles per step, directly after that
    step's ensemble_feed, handed four groups with targets and a pose and three without targets.  Without ``quantiles``: the list a
    backend written before the op records.  The graph key ends ("samples", N), ("quantiles", (...))."""
    model, _, inputs, av = E.case("cpu")
    x, pose = [inputs[0], inputs[1]], inputs[2]

    def record(backend, **kw):
        rec = EE.ShapeRecorder(backend)
        ops.set_backend(rec)
        eng = MVAEInference(model, use_graph=False)
        keys, run = [], eng._run
        eng._run = lambda key, fn, args: (keys.append(key), run(key, fn, args))[1]
        eng.noise = InjectedNoise(EE.blocks(N), [])
        del rec.ops[:], rec.sigs[:]
        eng.rollout(x, pose=pose, steps=T, available=av, sample=True, samples=N, **kw)
        eng.close()
        return list(rec.ops), list(rec.sigs), keys[0]
    Q = len(QS)
    image = ((N * B, 3, 64, 64), (Q, B, 3, 64, 64))
    for kw, extra in ((dict(), ()), (dict(targets=RC.frames(905)), ((N * B,), (Q, B)))):
        before, sigs_before, key_before = record(EmuBackendEnsemble(), **kw)
        plain, _, key_plain = record(EmuBackendQuantiles(), **kw)
        assert plain == before and key_plain == key_before and key_plain[-1] == ("samples", N)
        names, sigs, key = record(EmuBackendQuantiles(), quantiles=QS, **kw)
        want = []
        for name in before:
            want += [name, "ensemble_quantiles"] if name == "ensemble_feed" else [name]
        assert names == want and names.count("ensemble_quantiles") == T == before.count("ensemble_feed")
        assert [s for s in sigs if s[0] != "ensemble_quantiles"] == sigs_before
        for s in sigs:
            if s[0] == "ensemble_quantiles":
                assert s[1] == image + image + ((N * B, 7), (Q, B, 7)) + extra, s
        assert key[:-1] == key_plain and key[-2:] == (("samples", N), ("quantiles", QS))
    # the order and the type of the q values are the caller's: another order is another key
    _, _, key = record(EmuBackendQuantiles(), quantiles=[1, 0.5])
    assert key[-1] == ("quantiles", (1.0, 0.5)) and all(type(q) is float for q in key[-1][1])


def test_argument_errors():
    """8. Every ValueError of the argument, and a backend written before the op."""
    model, eng, inputs, av = E.case("cpu")
    x = [inputs[0], inputs[1]]
    roll = lambda **kw: eng.rollout(x, pose=inputs[2], steps=T, **kw)
    with pytest.raises(ValueError, match="quantiles needs samples"):
        roll(sample=True, quantiles=(0.5,))
    for bad in ((), [], (0.1,) * 9, 0.5, "0.5", torch.tensor([0.5])):
        with pytest.raises(ValueError, match="quantiles must be a sequence of 1 to 8"):
            roll(sample=True, samples=2, quantiles=bad)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "0.5", None, True):
        with pytest.raises(ValueError, match=r"numbers in \[0, 1\]"):
            roll(sample=True, samples=2, quantiles=(0.5, bad))
    with pytest.raises(ValueError, match=f"MMDYN_QUANTILE_N_MAX = {QC.QUANTILE_N_MAX}"):
        roll(sample=True, samples=QC.QUANTILE_N_MAX + 1, quantiles=(0.5,))
    with pytest.raises(ValueError, match="N identical trajectories"):
        roll(samples=2, quantiles=(0.5,))
    assert ops.QUANTILE_N_MAX == QC.QUANTILE_N_MAX >= 128 and ops.QUANTILES_MAX == QC.QUANTILES_MAX == 8
    ops.set_backend(EmuBackendEnsemble())
    eng.noise = InjectedNoise(EE.blocks(2), [])
    with pytest.raises(RuntimeError, match="ensemble_quantiles"):
        roll(sample=True, samples=2, quantiles=(0.5,))
    eng.close()


def test_emulated_op_follows_the_contract():
    """The emulation's rank counting against the sort of the restatement: ties, +-Inf, a NaN that stays in its element, and its
    argument errors."""
    emu, n, b = EmuBackendQuantiles(), 5, 3
    src = torch.randn(n * b, 6, generator=torch.Generator().manual_seed(7))
    src[0:3 * b:b, 0] = 0.25                                                  # three equal samples in element (0, 0)
    src[b, 1], src[2 * b, 1], src[3 * b, 2] = float("inf"), float("-inf"), float("inf")
    src[2 * b + 1, 4] = float("nan")
    qs = (0.0, 1.0, 0.5, 0.3, 0.3, 0.77)
    lo, frac = QC.index_of(qs, n)
    for logits in (False, True):
        out = torch.full((len(qs), b, 6), 7.0)
        emu.ensemble_quantiles([dict(src=src, out=out, logits=logits)], lo, frac, n, b)
        p = (torch.sigmoid(src) if logits else src).view(n, b, 6)
        assert QC.first_diff(out, QC.restate(p, lo, frac)) is None
        nan = torch.isnan(out)
        assert bool(nan[:, 1, 4].all()) and int(nan.sum()) == len(qs)          # the NaN sample: its element, all Q, nothing else
        assert float(out[0, 0, 1]) == (0.0 if logits else float("-inf")) and float(out[1, 0, 1]) == (1.0 if logits else float("inf"))
    g = lambda **k: dict(dict(src=src, out=torch.zeros(len(qs), b, 6), logits=False), **k)
    for groups, l, f, nn, bb in (([], lo, frac, n, b), ([g()] * 5, lo, frac, n, b), ([g()], lo[:2], frac, n, b),
                                 ([g()], [n] + lo[1:], frac, n, b), ([g()], lo, [1.0] + frac[1:], n, b),
                                 ([g()], lo, [float("nan")] + frac[1:], n, b), ([g()], lo, frac, n, b + 1),
                                 ([g()], lo, frac, QC.QUANTILE_N_MAX + 1, b), ([g(out=torch.zeros(len(qs), b, 5))], lo, frac, n, b),
                                 ([g()], lo * 2, frac * 2, n, b)):
        with pytest.raises(ValueError):
            emu.ensemble_quantiles(groups, l, f, nn, bb)


def test_hip_backend_validates_on_the_host():
    """HipBackend.ensemble_quantiles checks the groups, shapes, dtypes, contiguity, lo and frac before it touches the library, and
    refuses CPU tensors."""
    hip, n = ops.HipBackend(), 2
    f = lambda *s: torch.zeros(*s)
    g = lambda **k: dict(dict(src=f(n * B, 7), out=f(2, B, 7), logits=False), **k)
    lo, frac = [0, 1], [0.5, 0.0]
    shared = f(n * B + 2 * B, 7)
    for groups, l, fr, nn, rows in (([], lo, frac, n, B), ([g()] * 5, lo, frac, n, B), ([g(out=f(2, B, 8))], lo, frac, n, B),
                                    ([g(out=f(3, B, 7))], lo, frac, n, B), ([g(out=f(2, B + 1, 7))], lo, frac, n, B),
                                    ([g(src=f(n * B, 7).double())], lo, frac, n, B), ([g(out=f(2, B, 14)[:, :, ::2])], lo, frac, n, B),
                                    ([g(src=f(n * B, 0), out=f(2, B, 0))], lo, frac, n, B), ([g(src=None)], lo, frac, n, B),
                                    ([g()], [0, 2], frac, n, B), ([g()], [-1, 1], frac, n, B), ([g()], [0.0, 1], frac, n, B),
                                    ([g()], lo, [0.5, 1.0], n, B), ([g()], lo, [0.5, float("nan")], n, B),
                                    ([g()], lo, [0.5, -0.1], n, B), ([g()], lo, [0.5], n, B), ([g()], [], [], n, B),
                                    ([g()], [0] * 9, [0.0] * 9, n, B), ([g()], lo, frac, 0, B), ([g()], lo, frac, n, 0),
                                    ([g()], lo, frac, ops.QUANTILE_N_MAX + 1, B),
                                    ([g(src=shared[:n * B], out=shared[n * B - B:n * B + B].view(2, B, 7))], lo, frac, n, B)):
        with pytest.raises(ValueError):
            hip.ensemble_quantiles(groups, l, fr, nn, rows)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.ensemble_quantiles([g(), g(src=f(n * B), out=f(2, B))], lo, frac, n, B)


def test_problem_layer():
    """8. DynModeling.rollout(samples=2, quantiles=...): the argument reaches the engine, the new keys come back with their shapes,
    and the refusals pass through."""
    n, l = 2, 3
    model = TMM.build(False, "cpu")
    prob = TMM.problem_of(model, "cnn-mvae", False, "cpu", DynModeling)
    prob._seq_length, prob._kl_weight, prob._pose_multiplier = l, RC.KL_WEIGHT, RC.POSE_MULTIPLIER
    data, target = E.sequences(n, l)
    rec = prob._roller = E.RecordingEngine(model)
    prob.rollout(data, target, sample=True, samples=2, quantiles=(0.05, 0.95))
    prob.rollout(data, target, sample=True, samples=2)
    assert rec.calls[0]["quantiles"] == (0.05, 0.95) and rec.calls[0]["samples"] == 2 and "quantiles" not in rec.calls[1]
    del prob._roller
    res = prob.rollout(data, target, observe=("tactile",), sample=True, samples=2, quantiles=(0.05, 0.5, 0.95))
    assert set(res) == KEYS
    assert tuple(res["visual_q"].shape) == (l, 3, n, 3, 64, 64) == tuple(res["tactile_q"].shape)
    assert tuple(res["pose_q"].shape) == (l, 3, n, 7) and tuple(res["rows_q"].shape) == (l, 3, n)
    lo, frac = QC.index_of((0.05, 0.5, 0.95), 2)
    assert QC.first_diff(res["rows_q"], torch.stack([QC.restate(res["rows"][i], lo, frac) for i in range(l)])) is None
    assert QC.first_diff(res["visual_q"], restated(res["visual"], (0.05, 0.5, 0.95), 2)) is None   # vision is not observed
    prob._roller.close()
    with pytest.raises(ValueError, match="quantiles needs samples"):
        prob.rollout(data, target, sample=True, quantiles=(0.5,))
    with pytest.raises(ValueError, match=r"numbers in \[0, 1\]"):
        prob.rollout(data, target, sample=True, samples=2, quantiles=(1.5,))
