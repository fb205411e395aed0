"""The once form of the dense weight gradient (mmdyn_wgrad_tn_canon: one block per (channel tile, group) sums its row chunks itself
and writes the reference layout) against the two launches it stands in for (mmdyn_wgrad_tn / _grouped + mmdyn_wgrad_reduce).

1. Bit equality (`torch.equal`) on random normal operands, in fp32 and in the three-term split arithmetic, for every tile instance
   (LAB knob MMDYN_WGRAD_ONCE_TILE; a tile that does not divide the channels gives way to the next smaller one), with beta = 0 and
   with beta = 1 onto a non-zero canon.  The shapes are the smallest that take every branch: ragged last chunk, an empty chunk,
   cg_canon < Cg (unwritten columns), the three permutations, a grouped launch whose group boundary is no chunk boundary.  canon is a
   slice of a JUNK-filled buffer (exact_cases.Guarded) and, for cg_canon < Cg, is NaN before the beta = 0 launch: every element of
   [Cd][cg_canon] is written and nothing else.
2. Integer operands (exact_cases.ints): every partial sum is exact in fp32, the result equals canon_ref of the fp64 product bit for
   bit, in the three permutations.
3. The train step at B = 5 and B = 130, two steps in fp32x3 and in fp32, with layers.WGRAD_ONCE on and off: loss, the seven
   partials, every parameter and Adam moment and every BatchNorm buffer hold the same bits.

There is no tolerance in this file."""
import pytest
import torch

import exact_cases as X
from exact_cases import WGeo, canon_ref, ints, Guarded, check_exact
from mmdyn_hip import _lib, layers, ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import NoiseSource
from mmdyn_hip.ops import DENSE
from mmdyn_hip.utils.seeded_init import seeded_batch
import test_model_emu as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.HipBackend()
HIP_LAB = ops.HipBackend(lib_path=_lib.LAB_LIB_PATH)
TILES = ["128x128", "128x64", "64x64"]

# (G, rows per group, Cd, Cg, cg_canon, perm, chunks the cut gives)
CASES = [
    (1, 300, 128, 6400, 6400, 1, 4),       # chunks of 96 / 96 / 96 / 12 rows
    (1, 130, 64, 6400, 6400, 1, 4),        # 64 / 64 / 2 / 0 rows: an empty chunk (the engine's B = 130)
    (1, 1100, 6400, 64, 40, 2, 8),         # ragged, columns 40..63 written nowhere
    (1, 1024, 512, 512, 512, 0, 8),
    (3, 257, 64, 512, 512, 0, 4),          # grouped: 96 / 96 / 65 / 0 rows per group, a group boundary inside a K-step
]


@pytest.fixture(params=["fp32", "fp32x3"])
def arith(request):
    for be in (HIP, HIP_LAB):
        be.precision, be.fp32_split = "fp32", request.param == "fp32x3"
    yield request.param
    for be in (HIP, HIP_LAB):
        be.precision, be.fp32_split = "fp32", False


def normal(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def two_launches(be, D, Gt, canon, G, rows, Cd, Cg, cgc, perm, chunks, beta):
    partial = torch.empty(chunks, G, Cd, Cg, device=DEV)
    if G == 1:
        be.wgrad_tn(D, Gt, partial, DENSE, rows, 1, 1, Cd, 1, 1, Cg, 1, 0, chunks)
    else:
        be.wgrad_tn_grouped(D, Gt, partial, G, rows, Cd, Cg, chunks)
    be.wgrad_reduce(partial, canon, chunks, 1, G * Cd, Cg, cgc, perm, beta)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", CASES)
def test_same_bits_as_gemm_and_reduce(case, tile, arith, monkeypatch):
    G, rows, Cd, Cg, cgc, perm, want_chunks = case
    monkeypatch.setenv("MMDYN_WGRAD_ONCE_TILE", tile)
    be = HIP_LAB
    chunks = be.wgrad_chunks(DENSE, rows, Cd, Cg)
    assert chunks == want_chunks and be.wgrad_canon_served(rows, Cd, Cg, G)
    D, Gt = normal((G * rows, Cd), 1), normal((G * rows, Cg), 2)
    what = f"{case} tile {tile} {arith}"
    ref, got = Guarded(G * Cd, cgc, torch.float32, DEV), Guarded(G * Cd, cgc, torch.float32, DEV)
    if cgc < Cg:
        ref.t.fill_(float("nan"))
        got.t.fill_(float("nan"))
    two_launches(be, D, Gt, ref.t, G, rows, Cd, Cg, cgc, perm, chunks, 0.0)
    be.wgrad_tn_canon(D, Gt, got.t, G, rows, Cd, Cg, cgc, perm, 0.0, chunks)
    torch.cuda.synchronize()
    got.check(f"{what}: canon")
    assert not torch.isnan(got.t).any(), f"{what}: elements of [Cd][cg_canon] left unwritten"
    assert torch.equal(got.t, ref.t), f"{what}: beta = 0"
    assert float(got.t.abs().max()) > 0
    # beta = 1 onto a non-zero canon
    base = normal((G * Cd * cgc,), 3)
    ref.t.copy_(base)
    got.t.copy_(base)
    two_launches(be, D, Gt, ref.t, G, rows, Cd, Cg, cgc, perm, chunks, 1.0)
    be.wgrad_tn_canon(D, Gt, got.t, G, rows, Cd, Cg, cgc, perm, 1.0, chunks)
    torch.cuda.synchronize()
    got.check(f"{what}: canon (beta = 1)")
    assert torch.equal(got.t, ref.t), f"{what}: beta = 1"
    assert not torch.equal(got.t, base)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 1 and c[1] != 300], ids=lambda c: f"perm{c[5]}")
def test_exact_integers(case, arith):
    G, rows, Cd, Cg, cgc, perm, _ = case
    w = WGeo((DENSE, rows, 1, Cd, 1, Cg, 1, 0, cgc, perm))
    D, Gt = ints((rows, Cd), 51), ints((rows, Cg), 52)
    assert float(X.wgrad_ref(w, D.abs(), Gt.abs()).max()) < X.LIMIT
    want = canon_ref(w, X.wgrad_ref(w, D, Gt))
    canon = Guarded(Cd, cgc, torch.float32, DEV)
    chunks = HIP.wgrad_chunks(DENSE, rows, Cd, Cg)
    assert HIP.wgrad_canon_served(rows, Cd, Cg)
    HIP.wgrad_tn_canon(D.to(DEV), Gt.to(DEV), canon.t, 1, rows, Cd, Cg, cgc, perm, 0.0, chunks)
    torch.cuda.synchronize()
    canon.check(f"{case} {arith}: canon")
    check_exact(canon.values().reshape(-1), want, f"{case} {arith}: canon (perm {perm}, cg_canon {cgc})", bitwise=True)


# ---- the train step -------------------------------------------------------------------------------------------------------------
class Counting:
    """Forwards everything to the wrapped backend (attribute writes included) and counts the calls by name."""

    def __init__(self, inner):
        object.__setattr__(self, "_inner", inner)
        object.__setattr__(self, "n", {})

    def __getattr__(self, attr):
        fn = getattr(self._inner, attr)
        if not callable(fn):
            return fn

        def wrapped(*a, **k):
            self.n[attr] = self.n.get(attr, 0) + 1
            return fn(*a, **k)
        return wrapped

    def __setattr__(self, attr, value):
        setattr(self._inner, attr, value)


def run_step(B, precision, on, monkeypatch):
    monkeypatch.setattr(layers, "WGRAD_ONCE", on)
    rec = Counting(ops.B)
    old = ops.set_backend(rec)
    try:
        m = T.build("cnn-mvae", True, True, DEV)
        step = MVAEStep(m, noise=NoiseSource(11), precision=precision)
        inputs, targets = seeded_batch(B, 5)
        gi, gt = [x.to(DEV) for x in inputs], [x.to(DEV) for x in targets]
        out = []
        for _ in range(2):
            loss = step.train_step(gi, gt, 0.02)
            out.append((loss.detach().clone().reshape(-1), step.partials[:7].clone()))
        torch.cuda.synchronize()
        state = dict(params=step.params.flat.clone(), adam_m=step.adam_m.clone(), adam_v=step.adam_v.clone())
        for k, b in m.named_buffers():
            state["buffer " + k] = b.detach().clone()
        step.close()
    finally:
        ops.set_backend(old)
    return out, state, rec.n


@pytest.mark.parametrize("precision", ["fp32x3", "fp32"])
@pytest.mark.parametrize("B", [5, 130])
def test_two_steps_equal_with_the_switch_on_and_off(B, precision, monkeypatch):
    on, s_on, n_on = run_step(B, precision, True, monkeypatch)
    off, s_off, n_off = run_step(B, precision, False, monkeypatch)
    # what ran: the "on" run wrote weight gradients through the once form, and has that many fewer GEMM + reduce pairs
    assert n_off.get("wgrad_tn_canon", 0) == 0 and n_on.get("wgrad_tn_canon", 0) > 0
    assert n_on["wgrad_tn"] + n_on["wgrad_tn_canon"] == n_off["wgrad_tn"]
    assert n_on["wgrad_reduce"] + n_on["wgrad_tn_canon"] == n_off["wgrad_reduce"]
    for s, ((l1, p1), (l0, p0)) in enumerate(zip(on, off)):
        assert torch.isfinite(l1).all()
        assert torch.equal(l1, l0), (s, float(l1), float(l0))
        assert torch.equal(p1, p0), (s, p1.tolist(), p0.tolist())
    assert set(s_on) == set(s_off) and any(k.startswith("buffer ") for k in s_on)
    for k in s_on:
        assert torch.equal(s_on[k], s_off[k]), (k, float((s_on[k].double() - s_off[k].double()).abs().max()))
