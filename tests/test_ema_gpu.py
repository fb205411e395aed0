"""The exponential moving average of the parameters on a real MI355X: mmdyn_ema_update per element against fp64 (bound derived
below), on a 4-byte aligned view and between guard elements; mmdyn_ema_tick against numpy fp64 bit for bit; the fused
mmdyn_adam_step_ema against the separate launches bit for bit (plain, clipped, guarded) and through skipped steps;
MVAEStep(ema_decay) eager against graph replay and against the recurrence over parameter snapshots; MVAEInference on the averaged
model."""
import math

import pytest
import torch

from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference, MVAEStep
from mmdyn_hip.models import NoiseSource
from mmdyn_hip.utils.seeded_init import seeded_batch
from dirty import JUNK, bits, fill_
from emu_backend_ema import tick_values
import test_model_emu as T

pytestmark = pytest.mark.gpu

HIP = ops.HipBackend()
DEV = "cuda"
F64 = torch.float64
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
D = 0.9


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def exact_sumsq(x):
    return float((x.double().cpu() ** 2).sum())


def ticked(d=D, warmup=False):
    st = ops.new_ema_state(d, warmup, DEV)
    HIP.ema_tick(st)
    return st


# ---- 1. the stand-alone update -------------------------------------------------------------------------------------------------
# n = 2^21 + 5 exceeds the element-wise grid cap (2048 blocks x 256 threads x 4): the grid-stride loop runs more than once
@pytest.mark.parametrize("n", [1, 3, 4, 100003, 2 ** 21 + 5])
def test_ema_update_per_element(n):
    """Every element within 3 * 2^-23 * max(|p|, |e|) of the fp64 value of e + (1 - d)(p - e): one rounding of p - e, one of the
    fmaf result, one of omd to fp32, each at most 2^-24 relative of a quantity bounded by 2 max(|p|, |e|)."""
    p0, e0 = rnd(n, seed=80), rnd(n, seed=81)
    st = ticked()
    omd = float(st[2])
    assert omd == 1.0 - D and float(st[0]) == 1.0
    want = e0.double() + omd * (p0.double() - e0.double())
    bound = 3 * 2.0 ** -23 * torch.maximum(p0.abs(), e0.abs()).double()
    guard = 8                                                           # (8 floats: the inner region stays 16-byte aligned)
    buf = fill_(torch.empty(n + 2 * guard, device=DEV), JUNK)
    e = buf[guard:guard + n]
    e.copy_(e0)
    p = p0.to(DEV)
    assert e.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0
    HIP.ema_update(e, p, st)
    got = e.cpu()
    err = (got.double() - want).abs()
    print(f"n {n}: largest used share of the bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), int((err > bound).nonzero()[0])
    if n > 4:
        assert not torch.equal(got, e0)
    junk = fill_(torch.empty(guard), JUNK)
    assert same_bits(buf[:guard], junk) and same_bits(buf[guard + n:], junk)        # nothing written outside ema[0:n]
    assert same_bits(p, p0)
    assert same_bits(st, ticked())                                      # the state is read, not written
    # 4-byte aligned views: dword accesses, the same bits -- the average alone, then both operands
    for shift_p in (False, True):
        big = fill_(torch.empty(n + 8, device=DEV), JUNK)
        big[1:n + 1] = e0.to(DEV)
        view = big[1:n + 1]
        pv = p
        if shift_p:
            bigp = torch.zeros(n + 8, device=DEV)
            bigp[3:n + 3] = p
            pv = bigp[3:n + 3]
            assert pv.data_ptr() % 16 == 12
        assert view.data_ptr() % 16 == 4
        HIP.ema_update(view, pv, st)
        assert same_bits(view, got), shift_p
        assert same_bits(big[:1], junk[:1]) and same_bits(big[n + 1:], junk[:7])


def test_ema_update_takes_an_empty_tensor_and_rejects_bad_arguments():
    st = ticked()
    empty = torch.zeros(4, device=DEV)[:0]
    HIP.ema_update(empty, empty, st)
    p = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError, match="alias"):
        HIP.ema_update(p, p, st)
    with pytest.raises(ValueError, match="as many elements"):
        HIP.ema_update(p[:4], p, st)
    with pytest.raises(ValueError):
        HIP.ema_update(torch.zeros(8, device=DEV), p, torch.zeros(3, dtype=F64, device=DEV))


# ---- 2. the tick -----------------------------------------------------------------------------------------------------------------
def test_ema_tick_is_numpy_fp64_bit_for_bit():
    d = 0.9999
    st = ops.new_ema_state(d, True, DEV)
    n = 0.0
    for _ in range(4):
        HIP.ema_tick(st)
        omd, n1 = tick_values(n, d, True)
        got = st.cpu()
        assert same_bits(got[2], torch.tensor(float(omd), dtype=F64)) and same_bits(got[0], torch.tensor(float(n1), dtype=F64))
        assert float(got[1]) == d and float(got[3]) == 1.0
        n = float(n1)
    assert [float(tick_values(k, d, True)[0]) for k in range(3)] == [1 - 0.1, 1 - 2 / 11, 0.75]    # (the warm-up is in force)
    st = ops.new_ema_state(d, False, DEV)
    HIP.ema_tick(st)
    assert float(st[2]) == 1.0 - d and float(st[0]) == 1.0
    # a guarded Adam state that says "skipped": nothing moves; "not skipped": the tick runs
    adam = torch.zeros(6, dtype=F64, device=DEV)
    adam[5] = 1.0
    before = st.clone()
    HIP.ema_tick(st, adam)
    assert same_bits(st, before)
    adam[5] = 0.0
    HIP.ema_tick(st, adam)
    assert float(st[0]) == 2.0


# ---- 3. fused equals separate ----------------------------------------------------------------------------------------------------
def _opt_state(n, seed):
    p0 = rnd(n, seed=seed)
    return p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)


def _measure(g, clip, ws, grad_scale, max_norm):
    HIP.grad_sumsq(g, ws, clip)
    HIP.grad_clip_coef(clip, grad_scale, max_norm)


def _separate(p, g, m, v, e, state, clip, es, grad_scale, guarded):
    if clip is None:
        HIP.adam_step(p, g, m, v, state, LR, B1, B2, EPS, grad_scale, guarded=guarded)
    else:
        HIP.adam_step_clipped(p, g, m, v, state, clip, LR, B1, B2, EPS, grad_scale, guarded=guarded)
    HIP.ema_tick(es, state if guarded else None)
    HIP.ema_update(e, p, es)


@pytest.mark.parametrize("form", ["plain", "clipped", "guarded", "guarded-clipped"])
@pytest.mark.parametrize("warmup", [False, True])
def test_fused_step_equals_adam_then_tick_then_update(form, warmup):
    n, grad_scale = 100003, 0.25
    clips, guarded = "clipped" in form, "guarded" in form
    g0 = rnd(n, seed=83) * 0.01
    max_norm = 0.5 * grad_scale * math.sqrt(exact_sumsq(g0))
    p, m, v = _opt_state(n, 84)
    pr, mr, vr = _opt_state(n, 84)
    e, er = p.clone(), pr.clone()
    ns = 6 if guarded else 3
    state, ref_state = torch.zeros(ns, dtype=F64, device=DEV), torch.zeros(ns, dtype=F64, device=DEV)
    es, ref_es = ops.new_ema_state(D, warmup, DEV), ops.new_ema_state(D, warmup, DEV)
    clip = torch.zeros(4, dtype=F64, device=DEV) if clips else None
    ws = torch.zeros(HIP.grad_sumsq_blocks(n), dtype=F64, device=DEV)
    for step in range(3):
        g = (g0 * (step + 1)).to(DEV)
        if clips:
            _measure(g, clip, ws, grad_scale, max_norm)
            assert float(clip[2]) < 1.0
        HIP.adam_step_ema(p, g, m, v, e, state, clip, es, LR, B1, B2, EPS, grad_scale, guarded=guarded)
        _separate(pr, g, mr, vr, er, ref_state, clip, ref_es, grad_scale, guarded)
        for name, a, b in (("p", p, pr), ("m", m, mr), ("v", v, vr), ("state", state, ref_state), ("ema", e, er),
                           ("ema_state", es, ref_es)):
            assert same_bits(a, b), (step, name)
        assert not same_bits(e, p)
    assert float(es[0]) == 3.0 and float(state[0]) == 3.0
    if clips:
        assert float(clip[3]) == 3.0


# ---- 4. the guard ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clips", [False, True])
def test_a_skipped_step_is_no_update_of_the_average(clips):
    """The inf / NaN sequence of test_guarded_clipped_adam_skips_a_step_whose_gradient_overflowed with the average on: a skipped
    step leaves ema and ema_state bit-identical, the finite steps equal the unguarded fused step, the count is that of the finite
    steps."""
    n = 100003
    g = rnd(n, seed=34) * 0.01
    max_norm = 0.5 * math.sqrt(exact_sumsq(g))
    p, m, v = _opt_state(n, 33)
    pr, mr, vr = _opt_state(n, 33)
    e, er = p.clone(), pr.clone()
    state, ref_state = torch.zeros(6, dtype=F64, device=DEV), torch.zeros(3, dtype=F64, device=DEV)
    es, ref_es = ops.new_ema_state(D, True, DEV), ops.new_ema_state(D, True, DEV)
    clip = torch.zeros(4, dtype=F64, device=DEV) if clips else None
    ref_clip = torch.zeros(4, dtype=F64, device=DEV) if clips else None
    ws = torch.zeros(HIP.grad_sumsq_blocks(n), dtype=F64, device=DEV)
    bad = g.clone()
    bad[n - 2] = float("inf")
    nan = g.clone()
    nan[7] = float("nan")
    finite_steps = 0
    for gg, finite in ((g, True), (bad, False), (g * 2, True), (nan, False), (g * 3, True)):
        before = (p.clone(), m.clone(), v.clone(), state[:3].clone(), e.clone(), es.clone())
        gd = gg.to(DEV)
        if clips:
            _measure(gd, clip, ws, 1.0, max_norm)
        HIP.adam_step_ema(p, gd, m, v, e, state, clip, es, LR, B1, B2, EPS, 1.0, guarded=True)
        if finite:
            finite_steps += 1
            if clips:
                _measure(gd, ref_clip, ws, 1.0, max_norm)
            HIP.adam_step_ema(pr, gd, mr, vr, er, ref_state, ref_clip, ref_es, LR, B1, B2, EPS, 1.0)
            assert same_bits(p, pr) and same_bits(m, mr) and same_bits(v, vr) and same_bits(state[:3], ref_state)
            assert same_bits(e, er) and same_bits(es, ref_es)
            assert not same_bits(e, before[4])
        else:
            assert same_bits(p, before[0]) and same_bits(m, before[1]) and same_bits(v, before[2])
            assert same_bits(state[:3], before[3])
            assert same_bits(e, before[4]) and same_bits(es, before[5])
        assert float(es[0]) == finite_steps
    assert float(state[0]) == 3.0 and float(state[4]) == 2.0 and float(es[0]) == 3.0


# ---- 5. the engine ---------------------------------------------------------------------------------------------------------------
def _run_engine(precision, use_pose, graphed, inputs, targets, steps=3, **kw):
    step = MVAEStep(T.build("cnn-mvae", True, use_pose, DEV), noise=NoiseSource(3), precision=precision, **kw)
    run = step.train_step_graphed if graphed else step.train_step
    snaps = [step.params.flat.clone()]
    for _ in range(steps):
        run(inputs, targets, 0.02)
        snaps.append(step.params.flat.clone())
    out = dict(flat=step.params.flat.clone(), m=step.adam_m.clone(), v=step.adam_v.clone(), snaps=snaps,
               skipped=step.skipped_steps, updates=step.ema_updates, ema=step.ema,
               norm=None if step.clip is None else float(step.clip[1]), clipped=step.clipped_steps)
    if step.ema_flat is not None:
        out.update(ema_flat=step.ema_flat.clone(), ema_state=step.ema_state.clone())
    step.close()
    return out


def _recurrence(snaps, d=D, warmup=False):
    e, st = snaps[0].clone(), ops.new_ema_state(d, warmup, DEV)
    for s in snaps[1:]:
        HIP.ema_tick(st)
        HIP.ema_update(e, s, st)
    return e, st


def _batch(B, use_pose):
    return (([x.to(DEV) for x in xs]) for xs in seeded_batch(B, 1234, with_pose=use_pose))


@pytest.mark.parametrize("precision,use_pose", [("fp32x3", True), ("fp32x3", False), ("fp16", True)])
def test_engine_keeps_the_average_eager_and_graphed_alike(precision, use_pose):
    B = 4
    inputs, targets = _batch(B, use_pose)
    eager = _run_engine(precision, use_pose, False, inputs, targets, ema_decay=D)
    graph = _run_engine(precision, use_pose, True, inputs, targets, ema_decay=D)
    for k in ("flat", "m", "v", "ema_flat", "ema_state"):
        assert same_bits(eager[k], graph[k]), k
    for r in (eager, graph):
        assert r["updates"] == 3 and r["skipped"] == 0
        want, st = _recurrence(r["snaps"])
        assert same_bits(r["ema_flat"], want) and same_bits(r["ema_state"], st)
        assert not same_bits(r["ema_flat"], r["flat"])
    # off: the engine as it was, and the average does not touch the step
    plain = _run_engine(precision, use_pose, False, inputs, targets)
    none = _run_engine(precision, use_pose, False, inputs, targets, ema_decay=None)
    assert none["ema"] is None and plain["ema"] is None and none["updates"] == 0
    for k in ("flat", "m", "v"):
        assert same_bits(plain[k], none[k]), k
        assert same_bits(plain[k], eager[k]), k


def test_engine_keeps_the_average_of_clipped_steps():
    """max_grad_norm (half the first step's norm, probed with max_grad_norm=inf) together with ema_decay."""
    B, precision, use_pose = 4, "fp32x3", True
    inputs, targets = _batch(B, use_pose)
    probe = _run_engine(precision, use_pose, False, inputs, targets, steps=1, max_grad_norm=float("inf"))
    first = probe["norm"]
    assert math.isfinite(first) and first > 0 and probe["clipped"] == 0
    clipped = _run_engine(precision, use_pose, False, inputs, targets, max_grad_norm=0.5 * first)
    eager = _run_engine(precision, use_pose, False, inputs, targets, max_grad_norm=0.5 * first, ema_decay=D, ema_warmup=True)
    graph = _run_engine(precision, use_pose, True, inputs, targets, max_grad_norm=0.5 * first, ema_decay=D, ema_warmup=True)
    for k in ("flat", "m", "v", "ema_flat", "ema_state"):
        assert same_bits(eager[k], graph[k]), k
    for k in ("flat", "m", "v"):
        assert same_bits(eager[k], clipped[k]), k
    assert eager["clipped"] == 3 and graph["clipped"] == 3 and eager["updates"] == 3 and graph["updates"] == 3
    want, st = _recurrence(eager["snaps"], warmup=True)
    assert same_bits(eager["ema_flat"], want) and same_bits(eager["ema_state"], st)


# ---- 6. serving the average ------------------------------------------------------------------------------------------------------
def _fresh_engine(sd, use_pose, forwards, x, pose):
    m = T.build("cnn-mvae", True, use_pose, DEV)
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    eng = MVAEInference(m.eval(), seed=11)
    for _ in range(forwards):                                           # (equal seeds, equal number of draws)
        out = [None if t is None else t.clone() for t in eng.forward(x, pose=pose)]
    eng.close()
    return out


def test_inference_engine_serves_the_average_and_follows_training():
    B, use_pose = 4, True
    inputs, targets = _batch(B, use_pose)
    step = MVAEStep(T.build("cnn-mvae", True, use_pose, DEV), noise=NoiseSource(3), precision="fp32x3", ema_decay=D)
    for _ in range(3):
        step.train_step(inputs, targets, 0.02)
    twin = step.ema_model()
    assert step.ema_model() is twin and not twin.training
    x, pose = inputs[:2], inputs[2]
    served = MVAEInference(twin, seed=11)
    got = [t.clone() for t in served.forward(x, pose=pose)]
    want = _fresh_engine(step.ema_state_dict(), use_pose, 1, x, pose)
    live = _fresh_engine(step.model.state_dict(), use_pose, 1, x, pose)
    for a, b in zip(got, want):
        assert same_bits(a, b)
    assert not same_bits(got[0], live[0]) and not same_bits(got[3], live[3])
    step.train_step(inputs, targets, 0.02)
    served.refresh()
    got2 = [t.clone() for t in served.forward(x, pose=pose)]
    want2 = _fresh_engine(step.ema_state_dict(), use_pose, 2, x, pose)
    for a, b in zip(got2, want2):
        assert same_bits(a, b)
    assert not same_bits(got2[3], got[3])
    assert step.ema_updates == 4
    served.close()
    step.close()
