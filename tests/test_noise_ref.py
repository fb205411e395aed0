"""CPU tests of the noise contract: the numpy Philox reference (tests/philox_ref.py) against the published
known-answer vectors, the range of the uniform mapping, the distribution the algorithm produces, and the counter
accounting of NoiseSource.  tests/test_noise_gpu.py compares the kernels with this reference element by element."""
import math

import numpy as np
import pytest
import torch

import philox_ref as P
from mmdyn_hip import ops
from mmdyn_hip.models import NoiseSource
from mmdyn_hip.models.shapes import DROPOUT_P

N_STAT = 1 << 20
SIGMAS = 5.0


# ------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------
# Random123 known-answer vectors for philox4x32-10: (counter words, key words, output words)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w[0]) for w in P.philox4x32_10_full(*ctr, *key))
    assert got == want


def test_kernel_layout_is_the_two_word_case():
    # counter {lo, hi, 0, 0}, key {seed lo, seed hi}; the position wraps at 2^64 and carries into the high word
    seed, off = (0x299f31d0 << 32) | 0xa4093822, (0x85a308d3 << 32) | 0x243f6a88
    full = P.philox4x32_10_full(0x243f6a88, 0x85a308d3, 0, 0, 0xa4093822, 0x299f31d0)
    assert [int(w) for w in P.words_ref(1, seed, off)[0]] == [int(w[0]) for w in full]
    w = P.words_ref(4, 0, 2 ** 32 - 2)
    for j, c in enumerate([(0xfffffffe, 0), (0xffffffff, 0), (0, 1), (1, 1)]):
        assert [int(x) for x in w[j]] == [int(x[0]) for x in P.philox4x32_10(c[0], c[1], 0, 0)]
    assert [int(x) for x in P.words_ref(2, 7, 2 ** 64 - 1)[1]] == [int(x[0]) for x in P.philox4x32_10(0, 0, 7, 0)]
    # the first Random123 vector is counter 0 of seed 0
    assert [int(x) for x in P.words_ref(1, 0, 0)[0]] == list(KAT[0][2])


# ------------------------------------------------------------------------------------------------
# the uniform mapping
# ------------------------------------------------------------------------------------------------
def test_u01_range():
    assert P.u01(0)[0] == np.float32(2.0 ** -25) == np.float32(P.U01_MIN)
    assert P.u01(0xffffffff)[0] == np.float32(1.0)          # 2^24 - 0.5 rounds to even: exactly 1, not below it
    # ... and so do the two below: x >> 8 = 2^24 - 2 and 2^24 - 3 both give 1 - 2^-23; 1 - 2^-24 is never produced
    assert P.u01(0xfffffeff)[0] == P.u01(0xfffffdff)[0] == np.float32(1.0) - np.float32(2.0 ** -23)
    assert P.u01(0xfffffcff)[0] == np.float32(1.0) - np.float32(2.0 ** -22)
    # the mapping only sees x >> 8: all 2^24 values, in chunks
    prev = np.float32(0.0)
    for lo in range(0, 1 << 24, 1 << 22):
        u = P.u01(np.arange(lo, lo + (1 << 22), dtype=np.uint64) << np.uint64(8))
        assert u.dtype == np.float32
        assert (u > 0).all() and (u <= 1).all()
        assert u[0] >= prev and (np.diff(u) >= 0).all()
        prev = u[-1]
    # the largest radius Box-Muller can produce from it
    assert math.sqrt(-2.0 * math.log(P.U01_MIN)) < P.RADIUS_MAX < math.sqrt(-2.0 * math.log(P.U01_MIN)) + 1e-4


# ------------------------------------------------------------------------------------------------
# the distribution (of the algorithm, not of the kernel)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_draws():
    z, radius = P.normal_ref(N_STAT, 99, 0)
    z.setflags(write=False)
    radius.setflags(write=False)
    return z, radius


def test_reference_is_standard_normal_cdf(ref_draws):
    z, radius = ref_draws
    assert np.isfinite(z).all() and (radius <= P.RADIUS_MAX).all() and (np.abs(z) <= radius).all()
    # The count of draws below x is Binomial(N, F(x)), sd sqrt(F (1 - F) / N).  The 2^-24 grid of the uniforms moves
    # P(radius > r) by at most one grid step, so F by at most 2^-24, which is added to the width.
    for x in np.arange(-4.0, 4.5, 0.5):
        F = 0.5 * math.erfc(-x / math.sqrt(2.0))
        got = float((z <= x).mean())
        width = SIGMAS * math.sqrt(F * (1.0 - F) / N_STAT) + 2.0 ** -24
        print(f"cdf x={x:+.1f} F={F:.6e} got={got:.6e} width={width:.2e}")
        assert abs(got - F) <= width, (x, got, F, width)


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_reference_draws_are_uncorrelated(ref_draws):
    z, _ = ref_draws
    # the sample correlation of m independent pairs is normal with sd 1 / sqrt(m) to first order
    r1 = _corr(z[:-1], z[1:])
    print(f"lag-1 correlation {r1:+.3e}, width {SIGMAS / math.sqrt(N_STAT - 1):.3e}")
    assert abs(r1) <= SIGMAS / math.sqrt(N_STAT - 1)
    lanes = z.reshape(-1, 4)
    m = lanes.shape[0]
    for a in range(4):
        for b in range(a + 1, 4):
            r = _corr(lanes[:, a], lanes[:, b])
            print(f"lanes {a},{b}: correlation {r:+.3e}, width {SIGMAS / math.sqrt(m):.3e}")
            assert abs(r) <= SIGMAS / math.sqrt(m), (a, b, r)
    # every lane is a unit-variance, zero-mean stream of its own: mean sd 1/sqrt(m), variance sd sqrt(2/m)
    for a in range(4):
        assert abs(float(lanes[:, a].mean())) <= SIGMAS / math.sqrt(m)
        assert abs(float(lanes[:, a].var()) - 1.0) <= SIGMAS * math.sqrt(2.0 / m)


@pytest.mark.parametrize("p_drop", [0.1, DROPOUT_P], ids=["0.1", "DROPOUT_P"])
def test_mask_keep_rate(p_drop):
    m = P.masks_ref(N_STAT, p_drop, 1234 ^ P.MASK_SEED_XOR, 0)
    assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
    p = float(np.float32(p_drop))
    # Binomial(N, 1 - p); the grid of the uniforms moves the keep probability by at most 2^-24
    width = SIGMAS * math.sqrt(p * (1.0 - p) / N_STAT) + 2.0 ** -24
    keep = float(m.mean())
    print(f"keep rate {keep:.6f} at p_drop {p_drop}: width {width:.2e}")
    assert abs(keep - (1.0 - p)) <= width
    assert P.masks_ref(64, 0.0, 5, 0).all()                     # u01 > 0: p_drop = 0 keeps everything


# ------------------------------------------------------------------------------------------------
# NoiseSource accounting
# ------------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for ops.B: notes (kind, seed, host offset, device base, numel) per draw and keeps the device counter
    on a CPU int64 tensor."""

    def __init__(self):
        self.draws, self.adds = [], []

    def random_normal(self, out, seed, offset, offset_dev=None):
        self.draws.append(("normal", seed, offset, int(offset_dev[0]) if offset_dev is not None else 0, out.numel()))

    def random_masks(self, masks, p_drop, seed, offset, offset_dev=None):
        assert p_drop == DROPOUT_P
        self.draws.append(("mask", seed, offset, int(offset_dev[0]) if offset_dev is not None else 0, masks.numel()))

    def counter_add(self, counter, inc):
        assert counter.dtype == torch.int64 and counter.numel() == 1
        self.adds.append(int(inc))
        counter += int(inc)


@pytest.fixture()
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops, "B", r)
    return r


def run_script(ns, script, device=torch.device("cpu")):
    outs = []
    for name, args in script:
        if name == "commit":
            ns.commit()
        else:
            outs.append(getattr(ns, name)(*args, device))
    return outs


def ranges(draws):
    """Absolute counter ranges [start, end) of recorded draws."""
    return [(off + base, off + base + P.counters_of(n)) for _, _, off, base, n in draws]


def assert_disjoint(rs):
    for i, (a0, a1) in enumerate(rs):
        assert a1 > a0
        for b0, b1 in rs[i + 1:]:
            assert a1 <= b0 or b1 <= a0, (rs,)


DRAWS = [("eps", ((3, 5, 7),)), ("keep_mask", ((2, 5, 9),)), ("eps_block", (2, 5, 7)), ("mask_block", (3, 7, 11)),
         ("eps", ((1,),)), ("keep_mask", ((5,),)), ("eps", ((2, 3),))]


def test_noise_source_draws_use_disjoint_counters(rec):
    seed = 11
    outs = run_script(NoiseSource(seed), DRAWS)
    assert [o.numel() % 4 for o in outs].count(0) == 0           # every count is ragged
    assert [tuple(o.shape) for o in outs] == [(3, 5, 7), (2, 5, 9), (2, 5, 7), (3, 7, 11), (1,), (5,), (2, 3)]
    assert [o.dtype for o in outs] == [torch.float32, torch.uint8, torch.float32, torch.uint8, torch.float32,
                                       torch.uint8, torch.float32]
    rs = ranges(rec.draws)
    assert_disjoint(rs)
    assert rs[0][0] == 0 and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))        # and leave no gap
    assert [d[4] for d in rec.draws] == [o.numel() for o in outs]
    for kind, s, *_ in rec.draws:
        assert s == (seed ^ 0x5DEECE66D if kind == "mask" else seed)
    assert (seed ^ 0x5DEECE66D) >> 32 != 0                       # the mask stream exercises the high key word
    assert rec.adds == []                                        # eager draws never touch the device counter


def test_noise_source_commit_moves_exactly_what_was_drawn(rec):
    ns = NoiseSource(3)
    ns.commit()                                                  # nothing drawn, no counter yet: nothing enqueued
    assert rec.adds == [] and ns.base is None
    run_script(ns, DRAWS[:3])
    drawn = sum(P.counters_of(d[4]) for d in rec.draws)
    assert ns.offset == drawn and int(ns.base[0]) == 0
    ns.commit()
    assert rec.adds == [drawn] and int(ns.base[0]) == drawn and ns.offset == ns._mark == 0
    ns.commit()                                                  # a second commit with nothing drawn
    assert rec.adds == [drawn] and int(ns.base[0]) == drawn and ns.offset == 0


def test_noise_source_continues_after_commit(rec):
    ns = NoiseSource(3)
    run_script(ns, DRAWS[:2] + [("commit", ())] + DRAWS[2:5] + [("commit", ())] + DRAWS[5:])
    rs = ranges(rec.draws)
    assert_disjoint(rs)
    starts = [r[0] for r in rs]
    assert starts == sorted(starts) and rs[0][0] == 0
    assert all(a[1] == b[0] for a, b in zip(rs, rs[1:]))         # the stream goes on where it stopped
    assert rec.adds == [rs[1][1], rs[4][1] - rs[1][1]]
    assert int(ns.base[0]) + ns.offset == rs[-1][1]


def test_noise_script_plan_matches_noise_source(rec):
    # the script the device test replays: the plan it checks against is what NoiseSource really asks the backend for
    run_script(NoiseSource(P.NOISE_SCRIPT_SEED), P.NOISE_SCRIPT)
    got = [(kind, seed, off + base, n) for kind, seed, off, base, n in rec.draws]
    assert got == P.noise_script_plan()
    assert [p[2] for p in got] == [0, 27, 50, 65] and rec.adds == [65]


# ------------------------------------------------------------------------------------------------
# the Box-Muller edge counters the device test launches at
# ------------------------------------------------------------------------------------------------
def test_edge_constants_reproduce():
    from test_noise_gpu import EDGE_SEED, EDGES
    T = 1 << 24
    kinds = set()
    for kind, counter, pair, first, second in EDGES:
        w = P.words_ref(1, EDGE_SEED, counter)[0]
        assert (int(w[2 * pair]) >> 8, int(w[2 * pair + 1]) >> 8) == (first, second), (kind, counter)
        kinds.add(kind)
        u = P.u01(w[2 * pair:2 * pair + 2])
        if kind == "u=1":
            assert first == T - 1 and u[0] == np.float32(1.0)
        elif kind == "u<1 (2^24-2)":                            # both round to 1 - 2^-23, the largest uniform below 1
            assert first == T - 2 and u[0] == np.float32(1.0) - np.float32(2.0 ** -23)
        elif kind == "u<1 (2^24-3)":
            assert first == T - 3 and u[0] == np.float32(1.0) - np.float32(2.0 ** -23)
        elif kind == "radius":
            assert first <= 3 and math.sqrt(-2.0 * math.log(float(u[0]))) > 5.5
        else:
            target = {"angle=0": 0, "angle=pi/2": 1 << 22, "angle=pi": 1 << 23, "angle=2pi": T - 1}[kind]
            assert abs(second - target) <= 4
    assert kinds == {"u=1", "u<1 (2^24-2)", "u<1 (2^24-3)", "radius", "angle=0", "angle=pi/2", "angle=pi", "angle=2pi"}
