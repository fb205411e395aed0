"""The on-device noise kernels (random_masks_kernel, random_normal_kernel, counter_add_kernel) and NoiseSource against
the exact numpy Philox reference (tests/philox_ref.py), element by element: masks bit for bit, normals within a bound
measured once on the MI355X.  Every training step, every captured-graph replay and the benchmark draw from these."""
import os
import re

import numpy as np
import pytest
import torch

import philox_ref as P
from mmdyn_hip import ops
from mmdyn_hip.models import NoiseSource
from mmdyn_hip.models.shapes import DROPOUT_P

pytestmark = pytest.mark.gpu

HIP = ops.HipBackend()
DEV = "cuda"

# Largest |z_gpu - z_ref| per element over the grid of test_normals_match_reference (all n, seeds and offsets below),
# measured on an MI355X (gfx950); the inputs are fixed, so the figure is deterministic (docs/LAB_NOTES.md).  The
# factor 4 only covers another compiler lowering of __logf, __cosf and __sinf.  Any structurally wrong kernel (a
# repeated word, a dropped counter or key word, a wrong offset or tail) errs by O(1), a sin/cos swap by O(radius).
NORMAL_ERR_MEASURED = 1.985464e-06   # at seed 0, offset 2^32 - 2, n = N_BIG; the Box-Muller edge launches stay below 2.3e-06
NORMAL_TOL = 4.0 * NORMAL_ERR_MEASURED


def ew_grid_cap():
    """The block cap of a grid-stride element-wise launch, read from csrc/common.h (ew_grid_cap)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "multimodal-dynamics_amd", "csrc", "common.h")).read()
    body = src[src.index("static inline int ew_grid_cap()"):]
    return int(re.search(r"return v > 0 \? v : (\d+);", body).group(1))


EW_BLOCK = 256
# one full trip of the grid-stride loop (cap * 256 threads, 4 elements each), then 257 counters of a second trip, the
# last of them ragged
N_BIG = 4 * ew_grid_cap() * EW_BLOCK + 1027
NS_SMALL = [1, 2, 3, 4, 5, 7, 1023, 1025]
P_DROPS = [0.0, 0.1, 0.5]
SEEDS = [0, 1234, 1234 ^ 0x5DEECE66D, 2 ** 63 + 5]
OFFSETS = [0, 7, 2 ** 32 - 2, 2 ** 40 + 1]
GUARD = 16
STREAMS = [pytest.param(s, o, id=f"seed{i}-off{j}") for i, s in enumerate(SEEDS) for j, o in enumerate(OFFSETS)]


def sizes(offset):
    # at 2^32 - 2 the third counter carries into the high counter word: n = 16 spans it
    return NS_SMALL + ([16] if offset == 2 ** 32 - 2 else []) + [N_BIG]


def draw_masks(n, p_drop, seed, offset, offset_dev=None):
    buf = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    HIP.random_masks(buf[:n], p_drop, seed, offset, offset_dev)
    buf = buf.cpu()
    assert (buf[n:] == 0xAB).all(), ("wrote past the end", n)
    return buf[:n]


GUARD_F = -777.25


def draw_normals(n, seed, offset, offset_dev=None):
    buf = torch.full((n + GUARD,), GUARD_F, dtype=torch.float32, device=DEV)
    HIP.random_normal(buf[:n], seed, offset, offset_dev)
    buf = buf.cpu()
    assert (buf[n:] == GUARD_F).all(), ("wrote past the end", n)
    return buf[:n]


def normal_err(z, n, seed, offset):
    """Largest per-element |z - z_ref|; every element finite and inside the radius the reference gives it."""
    assert z.dtype == torch.float32 and z.shape == (n,)
    assert torch.isfinite(z).all(), (n, seed, offset)
    ref, radius = P.normal_ref(n, seed, offset)
    err = np.abs(z.numpy().astype(np.float64) - ref)
    assert (radius <= P.RADIUS_MAX).all()
    return float(err.max())


def test_bound_is_tight_enough():
    assert ew_grid_cap() * EW_BLOCK * 4 < N_BIG               # a second grid-stride trip
    assert N_BIG % 4 != 0
    assert NORMAL_TOL < 1e-3


@pytest.mark.parametrize("seed,offset", STREAMS)
def test_masks_match_reference_bit_for_bit(seed, offset):
    for n in sizes(offset):
        u = P.uniforms_ref(n, seed, offset)
        for p_drop in P_DROPS:
            got = draw_masks(n, p_drop, seed, offset)
            want = torch.from_numpy(P.masks_ref(n, p_drop, seed, offset, uniforms=u))
            assert torch.equal(got, want), (n, p_drop, seed, offset, int((got != want).sum()))
            if p_drop == 0.0:
                assert bool(got.all())


@pytest.mark.parametrize("seed,offset", STREAMS)
def test_normals_match_reference(seed, offset):
    worst = 0.0
    for n in sizes(offset):
        err = normal_err(draw_normals(n, seed, offset), n, seed, offset)
        print(f"normal_err seed={seed} offset={offset} n={n} err={err:.6e}")
        worst = max(worst, err)
    print(f"normal_err_worst seed={seed} offset={offset} err={worst:.6e} tol={NORMAL_TOL:.3e}")
    assert worst <= NORMAL_TOL, (seed, offset, worst)


# Counters of seed 0 (found by scanning its first 2^24 counters with the reference) at which Box-Muller meets an edge:
# (kind, counter, pair within the counter, radius word >> 8, angle word >> 8).  tests/test_noise_ref.py recomputes
# the words.  x >> 8 = 2^24 - 1 gives u = 1.0 exactly (radius 0); 2^24 - 2 and 2^24 - 3 both round to 1 - 2^-23, the
# largest uniform below 1 that the mapping produces; x >> 8 <= 3 gives the largest radii; the angle words sit within
# 4 steps of 0, pi/2, pi and 2 pi.
EDGE_SEED = 0
EDGES = [
    ("u=1", 2330056, 1, 16777215, 15849840),
    ("u<1 (2^24-2)", 4826271, 0, 16777214, 4335896),
    ("u<1 (2^24-3)", 15848971, 0, 16777213, 12557690),
    ("radius", 10639176, 1, 1, 8961086),
    ("radius", 1767245, 0, 2, 11807634),
    ("angle=0", 5617470, 1, 16685178, 1),
    ("angle=pi/2", 7980426, 0, 10227027, 4194304),
    ("angle=pi/2", 620078, 1, 12421426, 4194303),
    ("angle=pi", 454764, 1, 7924407, 8388608),
    ("angle=pi", 474393, 0, 12974172, 8388606),
    ("angle=2pi", 7113731, 0, 5767465, 16777215),
    ("angle=2pi", 3960693, 0, 10339546, 16777213),
]


@pytest.mark.parametrize("kind,counter,pair,first,second", EDGES, ids=[f"{e[0]}@{e[1]}" for e in EDGES])
def test_box_muller_edges(kind, counter, pair, first, second):
    z = draw_normals(4, EDGE_SEED, counter)
    err = normal_err(z, 4, EDGE_SEED, counter)
    print(f"edge_err {kind} counter={counter} z={z.tolist()} err={err:.6e}")
    assert err <= NORMAL_TOL, (kind, z.tolist(), err)
    if kind == "u=1":                                          # radius 0: both members of the pair are +/-0
        assert float(z[2 * pair:2 * pair + 2].abs().max()) <= NORMAL_TOL


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("b", [5, 2 ** 33])
@pytest.mark.parametrize("a", [0, 7])
def test_device_offset_adds_to_host_offset(a, b):
    n, seed = 1025, 1234
    dev = torch.tensor([b], dtype=torch.int64, device=DEV)
    z_dev, z_host = draw_normals(n, seed, a, dev), draw_normals(n, seed, a + b)
    assert torch.equal(bits(z_dev), bits(z_host))
    assert normal_err(z_dev, n, seed, a + b) <= NORMAL_TOL
    m_dev, m_host = draw_masks(n, 0.5, seed, a, dev), draw_masks(n, 0.5, seed, a + b)
    assert torch.equal(m_dev, m_host)
    assert torch.equal(m_dev, torch.from_numpy(P.masks_ref(n, 0.5, seed, a + b)))
    assert int(dev.cpu()[0]) == b                              # the draws leave the counter alone


def test_counter_add_lands_exactly():
    inc = 2 ** 33 + 3
    c = torch.zeros(1, dtype=torch.int64, device=DEV)
    HIP.counter_add(c, inc)
    assert int(c.cpu()[0]) == inc
    HIP.counter_add(c, inc)
    assert int(c.cpu()[0]) == 2 * inc
    HIP.counter_add(c, 1)
    assert int(c.cpu()[0]) == 2 * inc + 1


@pytest.mark.parametrize("device", ["cuda", "cuda:0"])        # with and without the index: the counter must survive both
def test_noise_source_on_device(monkeypatch, device):
    monkeypatch.setattr(ops, "B", HIP)
    ns, outs = NoiseSource(P.NOISE_SCRIPT_SEED), []
    for name, args in P.NOISE_SCRIPT:
        if name == "commit":
            ns.commit()
        else:
            outs.append(getattr(ns, name)(*args, torch.device(device)))
    plan = P.noise_script_plan()
    assert len(outs) == len(plan) == 4
    assert int(ns.base.cpu()[0]) == plan[-1][2] and ns.offset == P.counters_of(plan[-1][3])
    for out, (kind, seed, pos, numel) in zip(outs, plan):
        flat = out.reshape(-1).cpu()
        assert out.numel() == numel
        if kind == "mask":
            assert torch.equal(flat, torch.from_numpy(P.masks_ref(numel, DROPOUT_P, seed, pos)))
        else:
            err = normal_err(flat, numel, seed, pos)
            print(f"noise_source_err pos={pos} n={numel} err={err:.6e}")
            assert err <= NORMAL_TOL, (pos, numel, err)
