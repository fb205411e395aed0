"""Clipping by the global L2 norm on a real MI355X: mmdyn_grad_sumsq (fp64 bound, determinism, dirty workspace, a 4-byte aligned
view, chaining), mmdyn_grad_clip_coef against numpy fp64, the clipped Adam / SGD steps bit for bit against the unclipped entry
points, and MVAEStep(max_grad_norm) eager against graph replay."""
import math

import numpy as np
import pytest
import torch

from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import NoiseSource
from mmdyn_hip.utils.seeded_init import seeded_batch
from dirty import NAN, JUNK, bits, fill_
import test_model_emu as T

pytestmark = pytest.mark.gpu

HIP = ops.HipBackend()
DEV = "cuda"
F64 = torch.float64
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def exact_sumsq(x):
    return float((x.double().cpu() ** 2).sum())                          # fp64 sum on the CPU of exact fp64 squares


def sumsq(g, ws=None, clip=None, accumulate=False):
    ws = torch.zeros(HIP.grad_sumsq_blocks(g.numel()), dtype=F64, device=DEV) if ws is None else ws
    clip = torch.zeros(4, dtype=F64, device=DEV) if clip is None else clip
    HIP.grad_sumsq(g, ws, clip, accumulate=accumulate)
    return clip


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# n = 2^21 + 5 exceeds the element-wise grid cap (2048 blocks x 256 threads x 4) of the other launches of the file
@pytest.mark.parametrize("n", [1, 3, 4, 100003, 2 ** 21 + 5])
def test_grad_sumsq(n):
    x = rnd(n, seed=70) * 0.01
    g = x.to(DEV)
    want = exact_sumsq(x)
    clip = sumsq(g)
    got = float(clip[0])
    print(f"n {n}: device {got!r} cpu fp64 {want!r} rel {abs(got - want) / want:.3e} bound {2 * n * 2.0 ** -53:.3e}")
    if n == 1:
        assert got == want                                              # one exact square, nothing to round
    # two fp64 summations of n exact non-negative terms: each within n 2^-53 of the true sum
    assert abs(got - want) <= 2 * n * 2.0 ** -53 * want
    assert same_bits(sumsq(g), clip)                                     # the same call twice
    nb = HIP.grad_sumsq_blocks(n)
    for fill in (NAN, JUNK):                                            # whatever the workspace held
        ws = fill_(torch.empty(nb + 3, dtype=F64, device=DEV), fill)
        assert same_bits(sumsq(g, ws=ws), clip), fill
        assert same_bits(ws[nb:], fill_(torch.empty(3, dtype=F64), fill))        # nothing written past the queried size
    big = torch.zeros(n + 8, device=DEV)
    big[1:n + 1] = g
    view = big[1:n + 1]
    assert view.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 0
    assert same_bits(sumsq(view), clip)                                  # 4-byte aligned only: the same bits
    # overwrite, not accumulate, by default; untouched entries stay
    dirty = torch.tensor([5.0, 6.0, 7.0, 8.0], dtype=F64, device=DEV)
    sumsq(g, clip=dirty)
    assert float(dirty[0]) == got and dirty[1:].tolist() == [6.0, 7.0, 8.0]


def test_grad_sumsq_chains_tensors_and_takes_an_empty_one():
    parts = [rnd(n, seed=71 + i) * 0.01 for i, n in enumerate((1, 7, 100003))]
    clip, ws = torch.zeros(4, dtype=F64, device=DEV), torch.zeros(HIP.grad_sumsq_blocks(100003), dtype=F64, device=DEV)
    for i, p in enumerate(parts):
        HIP.grad_sumsq(p.to(DEV), ws, clip, accumulate=i > 0)
    cat = torch.cat(parts)
    want, n = exact_sumsq(cat), cat.numel()
    assert abs(float(clip[0]) - want) <= 2 * n * 2.0 ** -53 * want
    # n == 0: S = 0, or unchanged when accumulating
    before = clip.clone()
    empty = torch.zeros(4, device=DEV)[:0]
    HIP.grad_sumsq(empty, ws, clip, accumulate=True)
    assert same_bits(clip, before)
    HIP.grad_sumsq(empty, ws, clip)
    assert float(clip[0]) == 0.0


def coef_ref(S, grad_scale, max_norm):
    with np.errstate(all="ignore"):
        norm = np.abs(np.float64(np.float32(grad_scale))) * np.sqrt(np.float64(S))
        c = np.float64(np.float32(max_norm)) / (norm + np.float64(1e-6))
    return float(norm), float(min(c, 1.0))


@pytest.mark.parametrize("case", ["below", "above", "inf", "zero", "scaled"])
def test_grad_clip_coef(case):
    g = (rnd(100003, seed=72) * 0.01).to(DEV)
    clip = sumsq(g)
    S = float(clip[0])
    grad_scale = 1.0 / 1024 if case == "scaled" else 1.0
    if case == "zero":
        clip[0] = S = 0.0
    norm0 = abs(grad_scale) * math.sqrt(S)
    max_norm = {"below": 2.0 * norm0, "above": 0.5 * norm0, "inf": float("inf"), "zero": 1.0, "scaled": 0.5 * norm0}[case]
    clip[3] = 41.0
    HIP.grad_clip_coef(clip, grad_scale, max_norm)
    norm, coef = coef_ref(S, grad_scale, max_norm)
    got = clip.cpu().tolist()
    print(case, got, norm, coef)
    assert got[0] == S
    # four IEEE operations (sqrt, multiply, add, divide), one ulp granted to each
    assert abs(got[1] - norm) <= 2.0 ** -50 * norm and abs(got[2] - coef) <= 2.0 ** -50 * coef
    clips = case in ("above", "scaled")
    assert (got[2] < 1.0) if clips else (got[2] == 1.0)
    assert got[3] == (42.0 if clips else 41.0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            HIP.grad_clip_coef(clip, 1.0, bad)


def _opt_state(n, seed):
    p0 = rnd(n, seed=seed)
    return p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)


def _measure(g, clip, ws, grad_scale, max_norm):
    HIP.grad_sumsq(g, ws, clip)
    HIP.grad_clip_coef(clip, grad_scale, max_norm)


def _factor(grad_scale, coef):
    return float(np.float32(np.float64(np.float32(grad_scale)) * np.float64(coef)))


@pytest.mark.parametrize("clips", [False, True])
def test_adam_step_clipped_is_adam_step_with_the_factor(clips):
    n, grad_scale = 100003, 0.25
    g0 = rnd(n, seed=73) * 0.01
    max_norm = (0.5 if clips else 2.0) * grad_scale * math.sqrt(exact_sumsq(g0))       # (of the smallest step's gradient)
    p, m, v = _opt_state(n, 74)
    pr, mr, vr = _opt_state(n, 74)
    state, ref_state = torch.zeros(3, dtype=F64, device=DEV), torch.zeros(3, dtype=F64, device=DEV)
    clip, ws = torch.zeros(4, dtype=F64, device=DEV), torch.zeros(HIP.grad_sumsq_blocks(n), dtype=F64, device=DEV)
    for step in range(3):
        g = (g0 * (step + 1)).to(DEV)
        _measure(g, clip, ws, grad_scale, max_norm if clips else max_norm * 3)
        coef = float(clip[2])
        assert (coef < 1.0) if clips else (coef == 1.0)
        HIP.adam_step_clipped(p, g, m, v, state, clip, LR, B1, B2, EPS, grad_scale)
        HIP.adam_step(pr, g, mr, vr, ref_state, LR, B1, B2, EPS, _factor(grad_scale, coef) if clips else grad_scale)
        for a, b in ((p, pr), (m, mr), (v, vr), (state, ref_state)):
            assert same_bits(a, b), step
    assert float(clip[3]) == (3.0 if clips else 0.0) and float(state[0]) == 3.0


def test_guarded_clipped_adam_skips_a_step_whose_gradient_overflowed():
    """The sequence of test_guarded_adam_skips_a_step_whose_gradient_overflowed, every finite step clipping: an inf or a NaN in the
    gradient leaves parameters, moments and step count untouched, counts a skipped step and no clipped one; the finite steps
    equal the unguarded clipped step."""
    n = 100003
    g = rnd(n, seed=34) * 0.01
    max_norm = 0.5 * math.sqrt(exact_sumsq(g))
    p, m, v = _opt_state(n, 33)
    pr, mr, vr = _opt_state(n, 33)
    state, ref_state = torch.zeros(6, dtype=F64, device=DEV), torch.zeros(3, dtype=F64, device=DEV)
    clip, ref_clip = torch.zeros(4, dtype=F64, device=DEV), torch.zeros(4, dtype=F64, device=DEV)
    ws = torch.zeros(HIP.grad_sumsq_blocks(n), dtype=F64, device=DEV)
    bad = g.clone()
    bad[n - 2] = float("inf")
    nan = g.clone()
    nan[7] = float("nan")
    for gg, finite in ((g, True), (bad, False), (g * 2, True), (nan, False), (g * 3, True)):
        before = (p.clone(), m.clone(), v.clone(), state[:3].clone(), float(clip[3]))
        gd = gg.to(DEV)
        _measure(gd, clip, ws, 1.0, max_norm)
        HIP.adam_step_clipped(p, gd, m, v, state, clip, LR, B1, B2, EPS, 1.0, guarded=True)
        if finite:
            _measure(gd, ref_clip, ws, 1.0, max_norm)
            HIP.adam_step_clipped(pr, gd, mr, vr, ref_state, ref_clip, LR, B1, B2, EPS, 1.0)
            assert same_bits(p, pr) and same_bits(m, mr) and same_bits(v, vr) and same_bits(state[:3], ref_state)
            assert float(clip[3]) == before[4] + 1
        else:
            assert not math.isfinite(float(clip[1]))
            assert same_bits(p, before[0]) and same_bits(m, before[1]) and same_bits(v, before[2])
            assert same_bits(state[:3], before[3]) and float(clip[3]) == before[4]
    assert float(state[0]) == 3.0 and float(state[4]) == 2.0 and float(clip[3]) == 3.0
    with pytest.raises(ValueError):
        HIP.adam_step_clipped(p, g.to(DEV), m, v, ref_state, clip, LR, B1, B2, EPS, 1.0, guarded=True)


@pytest.mark.parametrize("clips", [False, True])
def test_sgd_step_clipped_is_sgd_step_with_the_factor(clips):
    n, grad_scale = 100003, 0.25
    g0 = rnd(n, seed=75) * 0.01
    max_norm = (0.5 if clips else 6.0) * grad_scale * math.sqrt(exact_sumsq(g0))
    p, buf, _ = _opt_state(n, 76)
    pr, bufr, _ = _opt_state(n, 76)
    clip, ws = torch.zeros(4, dtype=F64, device=DEV), torch.zeros(HIP.grad_sumsq_blocks(n), dtype=F64, device=DEV)
    for step in range(3):
        g = (g0 * (step + 1)).to(DEV)
        _measure(g, clip, ws, grad_scale, max_norm)
        coef = float(clip[2])
        assert (coef < 1.0) if clips else (coef == 1.0)
        HIP.sgd_step_clipped(p, g, buf, clip, LR, 0.9, 5e-4, grad_scale, step == 0)
        HIP.sgd_step(pr, g, bufr, LR, 0.9, 5e-4, _factor(grad_scale, coef) if clips else grad_scale, step == 0)
        assert same_bits(p, pr) and same_bits(buf, bufr), step
    assert float(clip[3]) == (3.0 if clips else 0.0)


# ---- engine ----------------------------------------------------------------------------------------------------------------------
def _run_engine(precision, use_pose, max_grad_norm, graphed, inputs, targets, steps=3):
    step = MVAEStep(T.build("cnn-mvae", True, use_pose, DEV), noise=NoiseSource(3), precision=precision, max_grad_norm=max_grad_norm)
    run = step.train_step_graphed if graphed else step.train_step
    norms, grads = [], []
    for _ in range(steps):
        run(inputs, targets, 0.02)
        norms.append(step.clip[1].clone())
        grads.append(math.sqrt(exact_sumsq(step.params.grad)) / (step.world * (step._graph[2] if graphed else step.loss_scale)))
    out = dict(flat=step.params.flat.clone(), m=step.adam_m.clone(), v=step.adam_v.clone(), norms=torch.stack(norms), grads=grads,
               clipped=step.clipped_steps, skipped=step.skipped_steps, n=step.params.total)
    step.close()
    return out


@pytest.mark.parametrize("precision,use_pose", [("fp32x3", True), ("fp32x3", False), ("fp16", True)])
def test_engine_clips_eager_and_graphed_alike(precision, use_pose):
    """B = 4.  A first engine with max_grad_norm=inf measures the first step's norm; half of it clips all three steps (the norm does
    not halve within three Adam steps of lr 1e-3 -- and clipped_steps == 3 is asserted, not assumed)."""
    B = 4
    inputs, targets = (([x.to(DEV) for x in xs]) for xs in seeded_batch(B, 1234, with_pose=use_pose))
    probe = _run_engine(precision, use_pose, float("inf"), False, inputs, targets, steps=1)
    first = float(probe["norms"][0])
    assert math.isfinite(first) and first > 0 and probe["clipped"] == 0
    eager = _run_engine(precision, use_pose, 0.5 * first, False, inputs, targets)
    graph = _run_engine(precision, use_pose, 0.5 * first, True, inputs, targets)
    print(precision, use_pose, "norms", eager["norms"].tolist(), "of the buffer read back", eager["grads"])
    assert eager["clipped"] == 3 and graph["clipped"] == 3
    assert eager["skipped"] == 0 and graph["skipped"] == 0
    for k in ("flat", "m", "v", "norms"):
        assert same_bits(eager[k], graph[k]), k
    assert float(eager["norms"][0]) == first
    # the reported norm is that of the unscaled gradient (the buffer holds loss_scale times it in the fp16 modes); sqrt halves the
    # relative bound of the sum of squares
    for got, want in zip(eager["norms"].tolist(), eager["grads"]):
        assert abs(got - want) <= (eager["n"] * 2.0 ** -53 + 2.0 ** -51) * want
