"""Results must not depend on what the destination buffers held: every launch below runs on ZERO-, NaN- and JUNK-filled outputs
and workspaces (tests/dirty.py) and must give the same bits; the ZERO run is also held to the bound of the entry point's existing
test against the CPU emulation.  Workspaces the backend allocates itself (the persistent kernel's slabs, the column-sum scratch)
are dirtied through PoisonTorch on mmdyn_hip.ops; flag / ticket pools are state and stay zero.

The fp64 loss / KL sums are ACCUMULATORS (caller initialises; atomicAdd(double) in any order): they are started from 0 and from a
known value v and must satisfy  second == v + first  to rtol 1e-12 (the bound of test_bce_logits_groups_*), never bit equality.

Entry points of include/mmdyn_hip.h with a writable pointer that run_dirty does NOT launch here, and why:
  mmdyn_counter_add, mmdyn_adam_step, mmdyn_adam_step_guarded, mmdyn_sgd_step   pure state: in-place updates of caller-owned
        state (the optimizer runs in the engine-level schedule below: parameters and moments bit-identical);
  mmdyn_copy_many                                    a copy between caller-owned static buffers of a captured step (graphs are
        out of scope here); every destination byte is a source byte;
  mmdyn_resize_plan, mmdyn_resize_ksize, *_stat_tiles*, *_slab_floats*, *_chunks*, mmdyn_igemm_planes_served, mmdyn_version,
  mmdyn_abi_version                                  host queries.
mmdyn_dropout_expand takes neither `u`, `act` nor `planes` (only mmdyn_dropout_reduce does): launched as it is.
"""
import pytest
import torch
import torch.nn.functional as F

import test_kernels_gpu as K
from test_kernels_gpu import (IGEMM_CASES, WGRAD_CASES, WSP_CASES, D16_TILES, DEV, rnd, rel,                 # noqa: F401
                              lab, regstage, mfma16, wsp, d16_tile, store16, bf16_mode)                         # noqa: F401
from dirty import FILLS, JUNK, NAN, ZERO, PoisonTorch, _arg_names, assert_same_bits, run_dirty
from mmdyn_hip import engine, layers, ops
from mmdyn_hip._lib import MmdynError
from mmdyn_hip.ops import DENSE, CONV, TCONV_S2P1, IM2COL3, TCONV_S1P0

pytestmark = pytest.mark.gpu

PT = PoisonTorch(ZERO)


@pytest.fixture(autouse=True)
def poisoned_backend_allocations(monkeypatch):
    """HipBackend's own torch.empty (the slab workspace of a persistent launch, the column-sum scratch) follows the fill."""
    PT.set_fill(ZERO)
    monkeypatch.setattr(ops, "torch", PT)
    yield


_REF = {}


def emu_ref(name, args, outs, key):
    """The emulation's outputs for this call, computed once per (entry point, case, precision) and shared between the routes."""
    k = (name, key, K.EMU.precision, tuple(str(args[i].dtype) for i in outs))
    if k not in _REF:
        cpu = [a.clone() if torch.is_tensor(a) else a for a in args]
        getattr(K.EMU, name)(*cpu)
        _REF[k] = {i: cpu[i] for i in outs}
    return _REF[k]


def launch(name, args, outs, post=None, tol=2e-5, key=None, scratch=(), state=(), untouched=None, approx=()):
    """run_dirty on the HIP backend of the running test (the LAB library under a forcing fixture) + bit equality across the fills
    + the existing test's bound for the ZERO run against the emulation (key=None: no emulation of this call)."""
    runs = run_dirty(K.HIP, name, args, outs, scratch=scratch, state=state, untouched=untouched, device=DEV, on_fill=PT.set_fill)
    assert_same_bits(runs, approx=approx, what=f"{name}: ")
    if key is not None:
        ref = emu_ref(name, args, outs, key)
        names = _arg_names(K.HIP, name, len(args))
        for i in outs:
            g, c = runs[ZERO][names[i]], ref[i]
            if post:
                g, c = post(i, g), post(i, c)
            assert rel(g, c) <= tol, (name, names[i], rel(g, c))
    return runs


# ---- igemm_nt -------------------------------------------------------------------------------------------------------------------
def igemm_both_forms(case):
    mode, G, Bg, Hi, Cin, Ho, N, stride, offset = case
    Bt = G * Bg
    taps = 16 if mode not in (DENSE, IM2COL3) else 1
    if mode == IM2COL3:
        A = rnd(Bt, 3, Hi, Hi, seed=90)
        Bp = rnd(1, 32, 64, seed=91, scale=0.2)
        Bp[:, :, 48:] = 0
    else:
        A, Bp = rnd(Bt * Hi * Hi, Cin, seed=1), rnd(taps, N, Cin, seed=2, scale=0.2)
    bias = rnd(N, seed=3)
    C, Ca = torch.zeros(Bt * Ho * Ho, N), torch.zeros(Bt * Ho * Ho, N)
    T = K.HIP.igemm_stat_tiles(mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N)
    stats = torch.zeros(G, T, 2, N)
    post = lambda i, t: t.sum(1) if i == 5 else t
    # (the emulation writes the sums into tile 0 whatever the tile count of the route: compared through sum(1), one run per case)
    launch("igemm_nt", [A, Bp, None, C, None, stats, None, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, N, stride, offset, 0, 1], [3, 5],
          post, key=("stats", case))
    launch("igemm_nt", [A, Bp, bias, C, Ca, None, None, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, N, stride, offset, 1, 1], [3, 4],
          key=("both", case))


@pytest.mark.parametrize("case", IGEMM_CASES)
def test_igemm_nt(case):
    igemm_both_forms(case)


@pytest.mark.parametrize("case", IGEMM_CASES)
def test_igemm_nt_regstage(case, regstage):
    igemm_both_forms(case)


@pytest.mark.parametrize("case", IGEMM_CASES)
def test_igemm_nt_mfma16(case, mfma16):
    igemm_both_forms(case)


def wsp_pairs(cases):
    """(forced tile, case) pairs of the persistent route: only the cases whose N is a multiple of the forced tile width."""
    return [(t, c) for t in ("128,64", "128,128") for c in cases if c[6] % int(t.split(",")[1]) == 0]


@pytest.mark.parametrize("wsp,case", wsp_pairs(WSP_CASES), indirect=["wsp"])
def test_igemm_nt_persistent(case, wsp):
    """Every tile split between blocks: the slabs (poisoned through ops.torch.empty) are written before the fix-up reads them."""
    igemm_both_forms(case)


@pytest.mark.parametrize("d16_tile", D16_TILES, indirect=True)
@pytest.mark.parametrize("case", IGEMM_CASES)
def test_igemm_d16(case, d16_tile):
    igemm_both_forms(case)


@pytest.mark.parametrize("case", [(TCONV_S1P0, 4, 70, 5, 256, 8, 128, 1, 0), (TCONV_S1P0, 2, 200, 5, 256, 8, 128, 1, 0),
                                  (TCONV_S1P0, 1, 5, 5, 256, 8, 128, 1, 0)])
def test_s1p0_persistent(case, lab, monkeypatch):
    monkeypatch.setenv("MMDYN_WSP_MIN_UNITS", "0")
    igemm_both_forms(case)


@pytest.mark.parametrize("H,Cin,G,Bg", [(16, 64, 2, 3), (16, 64, 1, 1), (16, 64, 4, 37), (32, 32, 2, 3), (32, 32, 1, 5), (64, 32, 2, 2),
                                        (64, 32, 1, 3)])
def test_tconv_patch_kernel(H, Cin, G, Bg):
    igemm_both_forms((TCONV_S2P1, G, Bg, H, Cin, 2 * H, 32, 1, 0))


@pytest.mark.parametrize("G,Bg,H", [(1, 2, 64), (2, 3, 64), (4, 8, 64), (2, 3, 32), (2, 3, 128), (2, 3, 256)])
def test_conv3_kernels(G, Bg, H):
    """The 3-channel layers (conv3.hip at 64 / 128 / 256 pixels, the tiled gather at 32): forward + statistics, the input gradient
    with the BatchNorm epilogue, the weight gradient at the recommended and at two other chunk counts."""
    Bt, Ho = G * Bg, H // 2
    igemm_both_forms((IM2COL3, G, Bg, H, 64, Ho, 32, 1, 0))
    x = rnd(Bt, 3, H, H, seed=90)
    Bp = rnd(1, 32, 64, seed=91, scale=0.2)
    Bp[:, :, 48:] = 0
    rows = Bt * Ho * Ho
    T = K.HIP.igemm_stat_tiles(IM2COL3, G, Bg, H, H, 64, Ho, Ho, 32)
    y = rnd(rows, 32, seed=92) * 1.5 + 0.2
    mean, rstd = rnd(G, 32, seed=93) * 0.3, rnd(G, 32, seed=94).abs() + 0.5
    gamma, beta = rnd(32, seed=95) + 1.2, rnd(32, seed=96)
    post = lambda i, t: t.sum(1) if t.dim() == 4 else t
    launch("igemm_nt_dgrad_bn", [x, Bp, torch.zeros(rows, 32), torch.zeros(G, T, 2, 32), y, mean, rstd, gamma, beta, IM2COL3, G, Bg, H, H,
                                64, Ho, Ho, 32, 1, 0], [2, 3], post, tol=5e-5, key=("c3", G, Bg, H, T))
    D = rnd(rows, 32, seed=97)
    for chunks in (K.HIP.wgrad_chunks(IM2COL3, rows, 32, 64), 4, 12):
        launch("wgrad_tn", [D, x, torch.zeros(chunks, 1, 32, 64), IM2COL3, Bt, Ho, Ho, 32, H, H, 64, 1, 0, chunks], [2],
              lambda i, t: t.sum(0), tol=5e-5, key=("c3", G, Bg, H, chunks))


@pytest.mark.parametrize("rows,Kd,N,splitk", [(256, 6400, 512, 25), (64, 512, 256, 3), (1024, 6400, 256, 8), (5, 64, 32, 2)])
def test_igemm_splitk(rows, Kd, N, splitk):
    A, Bp, bias = rnd(rows, Kd, seed=4), rnd(N, Kd, seed=5, scale=0.1), rnd(N, seed=6)
    ws = torch.zeros(splitk, rows, N)
    C = torch.zeros(rows, N)
    runs = launch("igemm_nt", [A, Bp, None, C, None, None, ws, DENSE, 1, rows, 1, 1, Kd, 1, 1, N, N, 1, 0, 0, splitk], [6],
                 lambda i, t: t.sum(0), key=("sk", rows, Kd, N, splitk))
    red = launch("splitk_reduce", [runs[ZERO]["ws"], bias, C, torch.zeros(rows, N), splitk, rows, N, 1], [2, 3], key=None)
    assert rel(red[ZERO]["C"], A @ Bp.t() + bias) < 2e-5


# ---- input-gradient GEMMs with an epilogue -------------------------------------------------------------------------------------
DGRAD_BN_CASES = [c for c in IGEMM_CASES if c[0] != DENSE][:6] + [IGEMM_CASES[0]]


def dgrad_bn(case, s16=None, tol=5e-5, all16=False):
    mode, G, Bg, Hi, Cin, Ho, N, stride, offset = case
    Bt, rows = G * Bg, G * Bg * Ho * Ho
    taps = 16 if mode != DENSE else 1
    cast = (lambda t: t.to(s16)) if s16 else (lambda t: t)
    A = cast(rnd(Bt * Hi * Hi, Cin, seed=31))
    Bp = rnd(taps, N, Cin, seed=32, scale=0.2)
    Bp = cast(Bp) if all16 else Bp
    y = cast(rnd(rows, N, seed=33) * 1.5 + 0.2)
    mean, rstd = rnd(G, N, seed=34) * 0.3, rnd(G, N, seed=35).abs() + 0.5
    gamma, beta = rnd(N, seed=36) + 1.2, rnd(N, seed=37)
    T = K.HIP.igemm_stat_tiles(mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, all16=all16)
    C, stats = torch.zeros(rows, N, dtype=s16 or torch.float32), torch.zeros(G, T, 2, N)
    post = lambda i, t: t.sum(1) if t.dim() == 4 else t.float()
    launch("igemm_nt_dgrad_bn", [A, Bp, C, stats, y, mean, rstd, gamma, beta, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, stride, offset],
          [2, 3], post, tol=tol, key=("dbn", case, T, all16))


def dgrad_act(case, act, s16=None, tol=5e-5, all16=False):
    mode, G, Bg, Hi, Cin, Ho, N, stride, offset = case
    Bt, rows = G * Bg, G * Bg * Ho * Ho
    taps = 1 if mode == DENSE else 16
    cast = (lambda t: t.to(s16)) if s16 else (lambda t: t)
    A, Bp = cast(rnd(Bt * Hi * Hi, Cin, seed=41)), rnd(taps, N, Cin, seed=42, scale=0.2)
    Bp = cast(Bp) if all16 else Bp
    u = cast(rnd(rows, N, seed=43) * 2.0)
    launch("igemm_nt_dgrad_act", [A, Bp, torch.zeros(rows, N, dtype=s16 or torch.float32), u, act, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N,
                                 stride, offset], [2], lambda i, t: t.float(), tol=tol, key=("dact", case, act, all16))


@pytest.mark.parametrize("case", DGRAD_BN_CASES)
def test_igemm_dgrad_bn(case):
    dgrad_bn(case)


@pytest.mark.parametrize("case", DGRAD_BN_CASES)
def test_igemm_dgrad_bn_regstage(case, regstage):
    dgrad_bn(case)


@pytest.mark.parametrize("case", DGRAD_BN_CASES)
def test_igemm_dgrad_bn_mfma16(case, mfma16):
    dgrad_bn(case)


@pytest.mark.parametrize("wsp,case", wsp_pairs([c for c in WSP_CASES if c[0] != DENSE]), indirect=["wsp"])
def test_igemm_dgrad_bn_persistent(case, wsp):
    dgrad_bn(case)


DGRAD_ACT_CASES = [IGEMM_CASES[2], IGEMM_CASES[3], IGEMM_CASES[5], IGEMM_CASES[6], IGEMM_CASES[8],
                   (TCONV_S2P1, 1, 3, 16, 64, 32, 32, 1, 0), (CONV, 1, 37, 8, 128, 5, 256, 1, 0)]


@pytest.mark.parametrize("case", DGRAD_ACT_CASES)
@pytest.mark.parametrize("act", [1, 2])
def test_igemm_dgrad_act(case, act):
    dgrad_act(case, act)


@pytest.mark.parametrize("wsp,case", wsp_pairs([WSP_CASES[2], WSP_CASES[4], WSP_CASES[-1], WSP_CASES[-2]]), indirect=["wsp"])
@pytest.mark.parametrize("act", [1, 2])
def test_igemm_dgrad_act_persistent(case, act, wsp):
    dgrad_act(case, act)


@pytest.mark.parametrize("case", [IGEMM_CASES[1], IGEMM_CASES[4], IGEMM_CASES[6], IGEMM_CASES[9], IGEMM_CASES[13]])
def test_igemm_16bit_storage(case, store16):
    """16-bit A and / or C (+ activated copy, + BatchNorm-backward operand): the outputs under store16, fp32 statistics."""
    mode, G, Bg, Hi, Cin, Ho, N, stride, offset = case
    Bt, rows = G * Bg, G * Bg * Ho * Ho
    taps = 16 if mode != DENSE else 1
    A, Bp, bias = K.bf(rnd(Bt * Hi * Hi, Cin, seed=41)), rnd(taps, N, Cin, seed=42, scale=0.2), rnd(N, seed=43)
    T = K.HIP.igemm_stat_tiles(mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N)
    post = lambda i, t: (t.sum(1) if t.dim() == 4 else t.float())
    for c_dtype in (K.S16, torch.float32):
        C, Ca, stats = torch.zeros(rows, N, dtype=c_dtype), torch.zeros(rows, N, dtype=c_dtype), torch.zeros(G, T, 2, N)
        tol = 4e-3 if c_dtype == K.S16 else 2e-5
        launch("igemm_nt", [A, Bp, None, C, None, stats, None, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, N, stride, offset, 0, 1], [3, 5], post,
              tol=tol, key=("s16", case, T))
        launch("igemm_nt", [A, Bp, bias, C, Ca, None, None, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, N, stride, offset, 1, 1], [3, 4], post,
              tol=tol, key=("s16b", case))
    dgrad_bn(case, s16=K.S16, tol=4e-3)


@pytest.mark.parametrize("wsp,case", wsp_pairs([(CONV, 2, 3, 16, 64, 8, 128, 2, -1), (CONV, 1, 37, 8, 128, 5, 256, 1, 0),
                                                 (TCONV_S2P1, 2, 5, 8, 128, 16, 64, 1, 0), (TCONV_S1P0, 2, 70, 5, 256, 8, 128, 1, 0),
                                                 (CONV, 4, 40, 16, 64, 8, 128, 2, -1)]), indirect=["wsp"])
def test_igemm_all16_persistent(case, wsp, store16, monkeypatch):
    """Both operands 16-bit on the persistent kernel, every tile split: 16-bit outputs, fp32 partial sums, dirty slabs."""
    mode, G, Bg, Hi, Cin, Ho, N, stride, offset = case
    monkeypatch.setenv("MMDYN_WSP_MIN_UNITS", "0")
    monkeypatch.setenv("MMDYN_WSP_B16", "1")
    Bt, rows = G * Bg, G * Bg * Ho * Ho
    A, Bp, bias = K.bf(rnd(Bt * Hi * Hi, Cin, seed=141)), K.bf(rnd(16, N, Cin, seed=142, scale=0.2)), rnd(N, seed=143)
    T = K.HIP.igemm_stat_tiles(mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, all16=True)
    post = lambda i, t: (t.sum(1) if t.dim() == 4 else t.float())
    for c_dtype in (K.S16, torch.float32):
        C, Ca, stats = torch.zeros(rows, N, dtype=c_dtype), torch.zeros(rows, N, dtype=c_dtype), torch.zeros(G, T, 2, N)
        tol = 4e-3 if c_dtype == K.S16 else 2e-5
        launch("igemm_nt", [A, Bp, None, C, None, stats, None, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, N, stride, offset, 0, 1], [3, 5], post,
              tol=tol, key=("a16", case, T))
        launch("igemm_nt", [A, Bp, bias, C, Ca, None, None, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, N, stride, offset, 1, 1], [3, 4], post,
              tol=tol, key=("a16b", case))
    if mode != TCONV_S1P0:
        y = K.bf(rnd(rows, N, seed=144) * 1.5 + 0.2)
        mean, rstd = rnd(G, N, seed=145) * 0.3, rnd(G, N, seed=146).abs() + 0.5
        gamma, beta = rnd(N, seed=147) + 1.2, rnd(N, seed=148)
        launch("igemm_nt_dgrad_bn", [A, Bp, torch.zeros(rows, N, dtype=K.S16), torch.zeros(G, T, 2, N), y, mean, rstd, gamma, beta, mode,
                                    G, Bg, Hi, Hi, Cin, Ho, Ho, N, stride, offset], [2, 3], post, tol=4e-3, key=("a16", case, T))
        launch("igemm_nt_dgrad_act", [A, Bp, torch.zeros(rows, N, dtype=K.S16), y, 1, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, stride, offset],
              [2], lambda i, t: t.float(), tol=4e-3, key=("a16", case))


# ---- fp32x3: in-kernel split and operands that arrive split --------------------------------------------------------------------
@pytest.fixture()
def x3():
    prev = K.HIP.fp32_split
    K.HIP.fp32_split = True
    yield
    K.HIP.fp32_split = prev


@pytest.mark.parametrize("planes", [False, True])
def test_x3_and_plane_launch(x3, planes):
    """The k4 s1 p0 layer at (G, Bg) = (4, 70) -- the smaller shape of the x3 / _planes tests of test_kernels_aten_gpu.py, served
    by the split's launch rule -- with statistics, against fp64 ATen at that file's bounds."""
    G, Bg = 4, 70
    B = G * Bg
    x, W = rnd(B, 256, 5, 5, seed=7), rnd(256, 128, 4, 4, seed=8, scale=0.1)
    Ws = torch.zeros(16 * 128 * 256)
    K.EMU.pack_conv_weight(W, Ws, 256, 128, 1)
    xr = x.permute(0, 2, 3, 1).reshape(-1, 256).contiguous()
    A, Bp = xr, Ws.view(16, 128, 256)
    if planes:
        assert K.HIP.igemm_planes_served(TCONV_S1P0, G, Bg, 5, 5, 256, 8, 8, 128)
        A, Bp = ops.Planes(xr.shape[0], 256, "cpu"), ops.Planes(16 * 128, 256, "cpu")
        for p, src in ((A, xr), (Bp, Ws.view(-1, 256))):
            hi = src.to(torch.bfloat16)
            mid = (src - hi.float()).to(torch.bfloat16)
            p.t[:, 0], p.t[:, 1], p.t[:, 2] = hi, mid, ((src - hi.float()) - mid.float()).to(torch.bfloat16)
    T = K.HIP.igemm_stat_tiles(TCONV_S1P0, G, Bg, 5, 5, 256, 8, 8, 128, planes=planes)
    runs = launch("igemm_nt", [A, Bp, None, torch.zeros(B * 64, 128), None, torch.zeros(G, T, 2, 128), None, TCONV_S1P0, G, Bg, 5, 5, 256,
                              8, 8, 128, 128, 1, 0, 0, 1], [3, 5])
    ref = F.conv_transpose2d(x.double(), W.double(), stride=1, padding=0)
    rr = ref.reshape(G, Bg, 128, 64).permute(0, 1, 3, 2).reshape(G, Bg * 64, 128)
    sums = runs[ZERO]["stats"].double().sum(1)
    assert float((sums[:, 0] - rr.sum(1)).norm() / rr.abs().sum(1).norm()) < 1e-6 and rel(sums[:, 1], (rr * rr).sum(1)) < 1e-5
    assert rel(runs[ZERO]["C"].view(B, 64, 128), ref.reshape(B, 128, 64).permute(0, 2, 1)) < 2e-6


# ---- weight gradients -----------------------------------------------------------------------------------------------------------
def wgrad(case, cast=None, chunks=None, key=None):
    mode, Bt, Hr, Cd, Hi, Cg, stride, offset = case
    rows, taps = Bt * Hr * Hr, 16 if mode == CONV else 1
    cast = cast or (lambda t: t)
    D, Gt = cast(rnd(rows, Cd, seed=7)), cast(rnd(Bt * Hi * Hi, Cg, seed=8))
    chunks = chunks or K.HIP.wgrad_chunks(mode, rows, Cd, Cg)
    return launch("wgrad_tn", [D, Gt, torch.zeros(chunks, taps, Cd, Cg), mode, Bt, Hr, Hr, Cd, Hi, Hi, Cg, stride, offset, chunks], [2],
                 lambda i, t: t.sum(0), tol=5e-5, key=("wg", case, chunks, key))


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad(case):
    wgrad(case[:8])


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad_bf16(case, bf16_mode):
    wgrad(case[:8])


@pytest.mark.parametrize("case", [(DENSE, 300, 1, 512, 1, 512, 1, 0), (CONV, 3, 8, 128, 16, 64, 2, -1), (CONV, 5, 5, 256, 8, 128, 1, 0),
                                  (CONV, 3, 16, 64, 32, 32, 2, -1), (CONV, 2, 8, 32, 16, 64, 2, -1), (DENSE, 77, 1, 256, 1, 6400, 1, 0)])
def test_wgrad_16bit_operands(case, store16):
    wgrad(case, cast=K.bf, key="s16")


def test_wgrad_im2col_16bit_dense_operand(store16):
    D, x = K.bf(rnd(2 * 1024, 32, seed=61)), rnd(2 * 3 * 64 * 64, seed=62)
    chunks = K.HIP.wgrad_chunks(IM2COL3, 2 * 1024, 32, 64)
    launch("wgrad_tn", [D, x, torch.zeros(chunks, 1, 32, 64), IM2COL3, 2, 32, 32, 32, 64, 64, 64, 1, 0, chunks], [2],
          lambda i, t: t.sum(0), tol=5e-5, key=("wgi", chunks))


@pytest.mark.parametrize("case", [(DENSE, 33, 1, 32, 1, 64, 1, 0), (DENSE, 70, 1, 512, 1, 512, 1, 0), (CONV, 1, 5, 256, 8, 128, 1, 0),
                                  (CONV, 3, 5, 64, 8, 32, 1, 0), (CONV, 1, 8, 128, 16, 64, 2, -1)])
def test_wgrad_with_empty_chunks(case):
    """More chunks than rows: rows_per_chunk is rounded up to the
    kernel's K-step, so late chunks start past `rows`.  That a chunk really was empty is read off the RESULT, not off constants of
    the kernel: a slab that saw a row of this random data is not all zero, so the launch must leave at least one all-zero slab --
    on NaN- and junk-filled memory too -- while the slabs still sum to the product.  Or the launch is refused: MMDYN_ERR_SHAPE."""
    mode, Bt, Hr, Cd = case[:4]
    rows = Bt * Hr * Hr
    chunks = max(4 * (rows // 4 + 2), K.HIP.wgrad_chunks(mode, rows, Cd, case[5]))
    assert chunks > rows                         # (whatever the K-step and the chunk grouping of a block: not every chunk gets a row)
    try:
        runs = wgrad(case, chunks=chunks)
    except MmdynError as e:                      # (_lib.check: "... failed: MMDYN_ERR_SHAPE ...")
        assert "SHAPE" in str(e), e
        return
    for fill in FILLS:
        empty = (runs[fill]["partial"].reshape(chunks, -1).abs().amax(1) == 0)
        assert int(empty.sum()) >= 1, fill


@pytest.mark.parametrize("Cd,Cg,Hr,Hi,stride,off", [(128, 64, 8, 16, 2, -1), (64, 64, 8, 16, 2, -1)])
def test_wgrad_on_operands_that_arrive_split(x3, Cd, Cg, Hr, Hi, stride, off):
    Bt = 6
    rows = Bt * Hr * Hr
    D, Gt = rnd(rows, Cd, seed=7), rnd(Bt * Hi * Hi, Cg, seed=8)

    def planes(src):
        p = ops.Planes(src.shape[0], src.shape[1], "cpu")
        hi = src.to(torch.bfloat16)
        mid = (src - hi.float()).to(torch.bfloat16)
        p.t[:, 0], p.t[:, 1], p.t[:, 2] = hi, mid, ((src - hi.float()) - mid.float()).to(torch.bfloat16)
        return p
    ref = emu_ref("wgrad_tn", [D, Gt, torch.zeros(4, 16, Cd, Cg), CONV, Bt, Hr, Hr, Cd, Hi, Hi, Cg, stride, off, 4], [2], ("pl", Cd, Cg))
    for pd, pg in ((True, True), (True, False), (False, True)):
        chunks = K.HIP.wgrad_chunks(CONV, rows, Cd, Cg, planes=(pd, pg))
        runs = launch("wgrad_tn", [planes(D) if pd else D, planes(Gt) if pg else Gt, torch.zeros(chunks, 16, Cd, Cg), CONV, Bt, Hr, Hr, Cd,
                                  Hi, Hi, Cg, stride, off, chunks], [2])
        assert rel(runs[ZERO]["partial"].sum(0), ref[2].sum(0)) <= 5e-5


@pytest.mark.parametrize("chunks,taps,Cd,Cg,cgc,perm", [(24, 16, 64, 32, 32, 0), (192, 16, 32, 32, 32, 0), (8, 1, 512, 6400, 6400, 1),
                                                        (8, 1, 6400, 256, 256, 2), (16, 1, 32, 64, 48, 0), (64, 16, 128, 64, 64, 0),
                                                        (68, 16, 128, 64, 64, 0), (8, 16, 64, 64, 48, 0)])
def test_wgrad_reduce(chunks, taps, Cd, Cg, cgc, perm):
    """beta = 0 into dirty `canon` (the guard `beta != 0 ? beta * canon : 0` is all that keeps a stale NaN out), both kernels (the
    one-pass kernel takes chunks <= 64 with slabs of >= 65536 floats), every permutation, cg_canon < Cg; beta = 1 from a known start."""
    partial = rnd(chunks, taps, Cd, Cg, seed=9)
    n = Cd * cgc * taps
    runs = launch("wgrad_reduce", [partial, torch.zeros(n), chunks, taps, Cd, Cg, cgc, perm, 0.0], [1], tol=5e-5,
                 key=("wr", chunks, taps, Cd, Cg, cgc, perm))
    start = rnd(n, seed=10)
    acc = launch("wgrad_reduce", [partial, start, chunks, taps, Cd, Cg, cgc, perm, 1.0], [], state=[1])
    assert rel(acc[ZERO]["canon"], start + runs[ZERO]["canon"]) <= 5e-5


# ---- small entry points ---------------------------------------------------------------------------------------------------------
def test_column_sums_and_small_linear(monkeypatch):
    for ticket in (False, True):
        monkeypatch.setattr(K.HIP, "force_ticket", ticket)
        launch("colsum", [rnd(300, 512, seed=24), torch.zeros(512), 300, 512, 0, 0.0], [1], key=("cs", 0))
        launch("colsum", [rnd(64, 6400, seed=25), torch.zeros(6400), 64, 6400, 2, 0.0], [1], key=("cs", 2))
        launch("colsum", [rnd(1000, 512, seed=62), torch.zeros(512), 1000, 512, 0, 0.0], [1], key=("cs", 3))
    monkeypatch.setattr(K.HIP, "force_ticket", False)
    launch("sum_blocks", [rnd(4, 999, seed=26), torch.zeros(999), 4, 999], [1], key="sb")
    for rows, Kd, N, act in [(33, 7, 512, 2), (33, 512, 7, 0)]:
        x, W, b = rnd(rows, Kd, seed=27), rnd(N, Kd, seed=28), rnd(N, seed=29)
        launch("linear_small_fwd", [x, W, b, torch.zeros(rows, N), rows, Kd, N, act], [3], key=("lf", Kd))
        launch("linear_small_bwd", [rnd(rows, N, seed=30), x, W, torch.zeros(rows, Kd), torch.zeros(N, Kd), torch.zeros(N), rows, Kd, N, 0.0],
              [3, 4, 5], key=("lb", Kd))


def test_scale_dev():
    """out = x * s[0] with s in device memory: no test at all before this one."""
    x, s = rnd(100003, seed=70) * 3, torch.tensor([-0.37])
    runs = launch("scale_dev", [x, s, torch.zeros(100003)], [2], tol=0.0, key="sd")
    assert torch.equal(runs[NAN]["out"], x * s)


@pytest.mark.parametrize("G,rpg,C", [(1, 1600, 256), (4, 700, 128), (2, 5000, 64), (3, 4096, 32), (1, 100, 256)])
def test_batchnorm_kernels(G, rpg, C, monkeypatch):
    y, da = rnd(G * rpg, C, seed=14) * 2 + 0.3, rnd(G * rpg, C, seed=15)
    gamma, beta = rnd(C, seed=16) + 1.5, rnd(C, seed=17)
    T = K.HIP.colstats_tiles(rpg)
    part = launch("colstats", [y, torch.zeros(G, T, 2, C), G, rpg, C], [1], lambda i, t: t.sum(1), key=("bn", G, rpg, C))[ZERO]["partial"]
    rm, rv, nbt = rnd(C, seed=18), rnd(C, seed=19).abs() + 0.5, torch.zeros((), dtype=torch.long)
    scratch = torch.zeros(32, G, 2, C, dtype=torch.float64)
    for ticket in (False, True):
        monkeypatch.setattr(K.HIP, "force_ticket", ticket)
        fin = run_dirty(K.HIP, "bn_finalize", [part, torch.zeros(G, C), torch.zeros(G, C), rm, rv, nbt, scratch, G, T, C, rpg, 1e-5, 0.1, 2],
                        [1, 2], scratch=[6], state=[3, 4, 5], device=DEV)
        assert_same_bits(fin, what="bn_finalize: ")
        cpu = [part.clone(), torch.zeros(G, C), torch.zeros(G, C), rm.clone(), rv.clone(), nbt.clone(), None, G, T, C, rpg, 1e-5, 0.1, 2]
        K.EMU.bn_finalize(*cpu)
        for name, i in (("mean", 1), ("rstd", 2), ("running_mean", 3), ("running_var", 4)):
            assert rel(fin[ZERO][name], cpu[i]) < 1e-5, name
        assert int(fin[JUNK]["nbt"]) == 2 * G
    monkeypatch.setattr(K.HIP, "force_ticket", False)
    mean, rstd = cpu[1], cpu[2]
    launch("bn_swish_fwd", [y, mean, rstd, gamma, beta, torch.zeros(G * rpg, C), G, rpg, C], [5], key=("bn", G, rpg, C))
    red = launch("bn_swish_bwd_reduce", [da, y, mean, rstd, gamma, beta, torch.zeros(G, T, 2, C), G, rpg, C], [6], lambda i, t: t.sum(1),
                tol=1e-4, key=("bn", G, rpg, C))[ZERO]["partial"]
    for ticket in (False, True):
        monkeypatch.setattr(K.HIP, "force_ticket", ticket)
        bwd = launch("bn_bwd_finalize", [red, torch.zeros(G, 2, C), torch.zeros(C), torch.zeros(C), scratch, G, T, C, 0.0], [1, 2, 3],
                    tol=1e-4, scratch=[4], key=("bn", G, rpg, C))
    monkeypatch.setattr(K.HIP, "force_ticket", False)
    launch("bn_swish_bwd_apply", [da, y, mean, rstd, gamma, beta, bwd[ZERO]["sums"], torch.zeros(G * rpg, C), G, rpg, C], [7], tol=1e-4,
          key=("bn", G, rpg, C))
    s64 = run_dirty(K.HIP, "bn_reduce_partials", [part, torch.zeros(G, 2, C, dtype=torch.float64), scratch, G, T, C], [1], scratch=[2],
                    device=DEV)
    assert_same_bits(s64, what="bn_reduce_partials: ")
    assert rel(s64[ZERO]["sums"], part.double().sum(1)) < 1e-6
    launch("bn_eval_stats", [rm, rv, torch.zeros(G, C), torch.zeros(G, C), G, C, 1e-5], [2, 3])


def test_elementwise_kernels():
    u, dh = rnd(1000, 513, seed=20) * 4, rnd(1000, 513, seed=21)
    for act in (0, 1, 2):
        launch("act_fwd", [u, torch.zeros_like(u), act], [1], key=("a", act))
        launch("act_bwd", [dh, u, torch.zeros_like(u), act], [2], key=("a", act))
    h = rnd(8, 512, seed=22)
    masks = (torch.rand(4, 8, 512, generator=torch.Generator().manual_seed(5)) > 0.1).to(torch.uint8)
    launch("dropout_expand", [h, masks, torch.zeros(4, 8, 512), 4, 8, 512, 0.1], [2], key="de")
    launch("dropout_reduce", [rnd(4, 8, 512, seed=23), masks, torch.zeros(8, 512), 4, 8, 512, 0.1], [2], key="dr")
    launch("dropout_reduce", [rnd(4, 8, 512, seed=23), masks, torch.zeros(8, 512), 4, 8, 512, 0.1, rnd(8, 512, seed=52) * 2, 1], [2],
          key="dru")


def test_elementwise_kernels_16bit(store16):
    G, rpg, C = 3, 1000, 64
    y, da = K.bf(rnd(G * rpg, C, seed=51) * 2 + 0.3), K.bf(rnd(G * rpg, C, seed=52))
    mean, rstd = rnd(G, C, seed=53) * 0.2, rnd(G, C, seed=54).abs() + 0.6
    gamma, beta = rnd(C, seed=55) + 1.5, rnd(C, seed=56)
    f32 = lambda i, t: t.float()
    launch("bn_swish_fwd", [y, mean, rstd, gamma, beta, torch.zeros(G * rpg, C, dtype=K.S16), G, rpg, C], [5], f32, tol=4e-3, key="e16")
    T = K.HIP.colstats_tiles(rpg)
    launch("bn_swish_bwd_reduce", [da, y, mean, rstd, gamma, beta, torch.zeros(G, T, 2, C), G, rpg, C], [6], lambda i, t: t.sum(1),
          tol=1e-4, key="e16")
    sums = emu_ref("bn_swish_bwd_reduce", [da, y, mean, rstd, gamma, beta, torch.zeros(G, T, 2, C), G, rpg, C], [6], "e16")[6].sum(1)
    launch("bn_swish_bwd_apply", [da, y, mean, rstd, gamma, beta, sums, torch.zeros(G * rpg, C, dtype=K.S16), G, rpg, C, False], [7], f32,
          tol=4e-3, key="e16")
    launch("act_bwd", [da, y, torch.zeros(G * rpg, C, dtype=K.S16), 1], [2], f32, tol=4e-3, key="e16")
    a = K.bf(rnd(2 * 32 * 32, 32, seed=57))
    launch("tconv_out3_fwd", [a, rnd(32, 3, 4, 4, seed=58, scale=0.2), torch.zeros(2, 3, 64, 64), 2, 32, 32], [2], key="e16")


def test_pack_and_layout_kernels():
    W = rnd(64, 32, 4, 4, seed=9)
    for swap in (0, 1):
        launch("pack_conv_weight", [W, torch.zeros(16 * 64 * 32), 64, 32, swap], [1], tol=0, key=("p", swap))
    for mode, ri, ci, ro, co in [(0, 32, 48, 32, 64), (1, 32, 48, 64, 32), (2, 8, 6400, 8, 6400), (3, 6400, 8, 6400, 8),
                                 (4, 8, 6400, 6400, 8), (5, 6400, 8, 8, 6400), (3, 6400, 1, 6400, 1)]:
        launch("repack2d", [rnd(ri, ci, seed=10), torch.zeros(ro * co), ri, ci, ro, co, mode], [1], tol=0, key=("r", mode, ci))
    x = rnd(3, 3, 64, 64, seed=11)
    launch("im2col_nchw3", [x, torch.zeros(3 * 1024 * 64), 3, 64, 64], [1], tol=0, key="i")
    launch("col2im_k4", [rnd(3 * 25, 2048, seed=12), torch.zeros(3 * 64 * 128), 3, 5, 5, 8, 8, 128, 2048, 1, 0, 1], [1], key="c1")
    launch("col2im_k4", [rnd(2 * 1024, 64, seed=13), torch.zeros(2 * 3 * 64 * 64), 2, 32, 32, 64, 64, 3, 64, 2, 1, 0], [1], key="c2")
    launch("nchw_to_nhwc", [x, torch.zeros(x.numel()), 3, 3, 4096], [1], tol=0, key="n1")
    launch("nhwc_to_nchw", [x, torch.zeros(x.numel()), 3, 3, 4096], [1], tol=0, key="n2")
    for Bt in (1, 5):
        launch("tconv_out3_fwd", [rnd(Bt * 32 * 32, 32, seed=60), rnd(32, 3, 4, 4, seed=61), torch.zeros(Bt, 3, 64, 64), Bt, 32, 32], [2],
              key=("t3", Bt))
    # a block written into a wider matrix: the pad columns ld > cols of each row are left untouched (include/mmdyn_hip.h)
    rows, cols, ld = 40, 500, 512
    mask = torch.zeros(rows, ld, dtype=torch.bool)
    mask[:, cols:] = True
    launch("repack2d_ld", [rnd(rows, cols, seed=102), torch.zeros(rows * ld), rows, cols, rows, cols, ld, 0], [1], tol=0,
          untouched={1: mask.reshape(-1)}, key="rl")
    src = rnd(100001, seed=3)
    c = launch("cast_f32_to_bf16", [src, torch.zeros(100001, dtype=torch.bfloat16)], [1], lambda i, t: t.float(), tol=0, key="cb")
    launch("cast_bf16_to_f32", [c[ZERO]["dst"], torch.zeros(100001)], [1], tol=0, key="cf")


def test_16bit_packs(store16):
    f32 = lambda i, t: t.float()
    Wc = rnd(128, 64, 4, 4, seed=101, scale=0.2)
    for swap in (0, 1):
        launch("pack_conv_weight", [Wc, torch.zeros(16, 64 if swap else 128, 128 if swap else 64, dtype=K.S16), 128, 64, swap], [1], f32,
              tol=0.0, key=("p16", swap))
    mask = torch.zeros(40, 512, dtype=torch.bool)
    mask[:, 500:] = True
    launch("repack2d_ld", [rnd(40, 500, seed=102), torch.zeros(40 * 512, dtype=K.S16), 40, 500, 40, 500, 512, 0], [1], f32, tol=0.0,
          untouched={1: mask.reshape(-1)}, key="rl16")


def test_random_kernels_into_dirty_destinations():
    n = 100003
    m = run_dirty(K.HIP, "random_masks", [torch.zeros(n, dtype=torch.uint8), 0.1, 1234, 0], [0], device=DEV)
    assert_same_bits(m, what="random_masks: ")
    assert set(m[JUNK]["masks"].unique().tolist()) <= {0, 1}
    z = run_dirty(K.HIP, "random_normal", [torch.zeros(n), 99, 0], [0], device=DEV)
    assert_same_bits(z, what="random_normal: ")


# ---- latent space and loss terms ------------------------------------------------------------------------------------------------
SUBSETS = [(1, 1, 0), (0, 1, 1), (1, 1, 1)]


def _passes(hs, ds, L, subsets):
    return [{"mu": [hs[m][:, :L] if s[m] else None for m in range(3)], "lv": [hs[m][:, L:] if s[m] else None for m in range(3)],
             "dmu": [ds[m][:, :L] if s[m] else None for m in range(3)], "dlv": [ds[m][:, L:] if s[m] else None for m in range(3)],
             "ld": [2 * L] * 3} for s in subsets]


def test_latent_kernels():
    """mu / logvar / z of the product of experts, and the dmu / dlv rows of the experts live in a pass; the gradient buffer of an
    expert absent from the pass is not handed to the kernel and must stay as it was (checked as a read-only argument).  kl_sum is
    an accumulator: v + first == second to rtol 1e-12, not bit equality (atomicAdd(double) adds in arrival order)."""
    B, L, P = 5, 256, 3
    heads = [rnd(B, 2 * L, seed=40 + i) for i in range(3)]
    dheads = [torch.zeros(B, 2 * L) for _ in range(3)]
    eps = torch.randn(P, B, L, generator=torch.Generator().manual_seed(5))

    def fwd(be, h0, h1, h2, d0, d1, d2, eps, mu, logvar, z, kl_sum):
        be.poe_fwd(_passes([h0, h1, h2], [d0, d1, d2], L, SUBSETS), eps, mu, logvar, z, kl_sum, 1, P, B, L)
    zeros = lambda: torch.zeros(P, B, L)
    outs = {}
    for v in (0.0, 1234.5):
        r = run_dirty(K.HIP, fwd, heads + dheads + [eps, zeros(), zeros(), zeros(), torch.full((P,), v, dtype=torch.float64)],
                      [7, 8, 9], state=[10], device=DEV)
        assert_same_bits(r, approx=("kl_sum",), what="poe_fwd: ")
        outs[v] = r[ZERO]
    assert torch.allclose(outs[1234.5]["kl_sum"], 1234.5 + outs[0.0]["kl_sum"], rtol=1e-12, atol=0)
    mu_c, lv_c, z_c, kl_c = zeros(), zeros(), zeros(), torch.zeros(P, dtype=torch.float64)
    K.EMU.poe_fwd(_passes(heads, dheads, L, SUBSETS), eps, mu_c, lv_c, z_c, kl_c, 1, P, B, L)
    for a, b in ((outs[0.0]["mu"], mu_c), (outs[0.0]["logvar"], lv_c), (outs[0.0]["z"], z_c), (outs[0.0]["kl_sum"], kl_c)):
        assert rel(a, b) < 1e-5
    dz = torch.randn(P, B, L, generator=torch.Generator().manual_seed(6))
    for p in range(P):
        def bwd(be, h0, h1, h2, d0, d1, d2, eps, mu, logvar, dz):
            be.poe_bwd(_passes([h0, h1, h2], [d0, d1, d2], L, SUBSETS[p:p + 1]), eps, mu, logvar, dz, None, None, 0.02 / B, 1, 1, B, L)
        live = [3 + m for m in range(3) if SUBSETS[p][m]]
        r = run_dirty(K.HIP, bwd, heads + dheads + [eps[p:p + 1].contiguous(), mu_c[p:p + 1].contiguous(), lv_c[p:p + 1].contiguous(),
                                                     dz[p:p + 1].contiguous()], live, device=DEV)
        assert_same_bits(r, what=f"poe_bwd pass {p}: ")
        dc = [torch.zeros(B, 2 * L) for _ in range(3)]
        K.EMU.poe_bwd(_passes(heads, dc, L, SUBSETS[p:p + 1]), eps[p:p + 1], mu_c[p:p + 1], lv_c[p:p + 1], dz[p:p + 1], None, None,
                      0.02 / B, 1, 1, B, L)
        for m in range(3):
            if SUBSETS[p][m]:
                assert rel(r[ZERO][f"d{m}"], dc[m]) < 1e-4, (p, m)

    def rfwd(be, h, eps, z, kl_sum):
        be.reparam_fwd(h[:, :L], h[:, L:], eps, z, kl_sum, B, L, 2 * L)
    got = {}
    for v in (0.0, -77.25):
        r = run_dirty(K.HIP, rfwd, [heads[0], eps[0].contiguous(), torch.zeros(B, L), torch.full((1,), v, dtype=torch.float64)], [2],
                      state=[3], device=DEV)
        assert_same_bits(r, approx=("kl_sum",), what="reparam_fwd: ")
        got[v] = r[ZERO]
    assert torch.allclose(got[-77.25]["kl_sum"], -77.25 + got[0.0]["kl_sum"], rtol=1e-12, atol=0)
    z1c, kl1c = torch.zeros(B, L), torch.zeros(1, dtype=torch.float64)
    K.EMU.reparam_fwd(heads[0][:, :L], heads[0][:, L:], eps[0], z1c, kl1c, B, L, 2 * L)
    assert rel(got[0.0]["z"], z1c) < 1e-5 and rel(got[0.0]["kl_sum"], kl1c) < 1e-6

    def rbwd(be, h, eps, dz, d):
        be.reparam_bwd(h[:, :L], h[:, L:], eps, dz, 0.3, d[:, :L], d[:, L:], B, L, 2 * L)
    r = run_dirty(K.HIP, rbwd, [heads[0], eps[0].contiguous(), dz[0].contiguous(), torch.zeros(B, 2 * L)], [3], device=DEV)
    assert_same_bits(r, what="reparam_bwd: ")
    dc = torch.zeros(B, 2 * L)
    K.EMU.reparam_bwd(heads[0][:, :L], heads[0][:, L:], eps[0], dz[0], 0.3, dc[:, :L], dc[:, L:], B, L, 2 * L)
    assert rel(r[ZERO]["d"], dc) < 1e-5


def _accumulates(name, args, outs, acc, v=4321.125, kwargs=None, names=None):
    """Gradient outputs bit-identical across the fills; the fp64 sums (state: started from 0 and from v) obey second == v + first
    to rtol 1e-12 -- they are atomicAdd(double) accumulators, whose order of addition differs from run to run."""
    got = {}
    for start in (0.0, v):
        call = list(args)
        for i in acc:
            call[i] = torch.full_like(args[i], start)
        r = run_dirty(K.HIP, name, call, outs, state=acc, device=DEV, kwargs=kwargs, names=names)
        assert_same_bits(r, approx=tuple(k for k in r[ZERO] if r[ZERO][k].dtype == torch.float64), what=f"{name}: ")
        got[start] = r[ZERO]
    for k, t in got[v].items():
        if t.dtype == torch.float64:
            assert torch.allclose(t, v + got[0.0][k], rtol=1e-12, atol=0), k
    return got[0.0]


def test_loss_kernels():
    n = 3 * 3 * 64 * 64
    logits, target = rnd(3, 3, 64, 64, seed=50) * 6, torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    mask = (torch.rand(3, 1, 64, 64, generator=torch.Generator().manual_seed(2)) > 0.5).float()
    for mk in (None, mask):
        g = _accumulates("bce_logits", [logits, target, mk, torch.zeros(n), torch.zeros(1, dtype=torch.float64), n, 3 * 4096, 4096, 0.25],
                         [3], [4])
        lc, dc = torch.zeros(1, dtype=torch.float64), torch.zeros(n)
        K.EMU.bce_logits(logits, target, mk, dc, lc, n, 3 * 4096, 4096, 0.25)
        assert rel(g["loss_sum"], lc) < 1e-6 and rel(g["dlogit"], dc) < 1e-5
    r, t = rnd(9, 7, seed=51), rnd(9, 7, seed=52)
    g = _accumulates("mse", [r, t, torch.zeros(63), torch.zeros(1, dtype=torch.float64), 63, 0.5], [2], [3])
    lc, dc = torch.zeros(1, dtype=torch.float64), torch.zeros(63)
    K.EMU.mse(r, t, dc, lc, 63, 0.5)
    assert rel(g["loss_sum"], lc) < 1e-6 and rel(g["dr"], dc) < 1e-6
    # the grouped launch: slot -1 is a discarded pass whose gradient rows are WRITTEN as zeros
    B, G = 5, 4
    n = B * 3 * 64 * 64
    lg, tg = rnd(G * n, seed=400) * 3, torch.rand(n, generator=torch.Generator().manual_seed(401))
    slots = [3, -1, 0, 5]
    g = _accumulates("bce_logits_groups", [lg, tg, torch.zeros(G * n), torch.zeros(8, dtype=torch.float64), slots, n, 0.2], [2], [3])
    cl, cd = torch.zeros(8, dtype=torch.float64), torch.zeros(G * n)
    K.EMU.bce_logits_groups(lg.clone(), tg.clone(), cd, cl, slots, n, 0.2)
    assert rel(g["dlogit"], cd) <= 2e-5 and torch.allclose(g["loss_slots"], cl, rtol=1e-5)
    assert float(g["dlogit"][n:2 * n].abs().max()) == 0.0
    for mask_c in (1, 3):
        mk = (torch.rand(B * mask_c * 4096, generator=torch.Generator().manual_seed(412)) > 0.35).float()
        un = torch.zeros(8, dtype=torch.float64)

        def masked(be, logits, target, dlogit, loss_slots, mask, unmasked_slots):
            be.bce_logits_groups(logits, target, dlogit, loss_slots, slots, n, 0.2, mask=mask, chw=3 * 4096, hw=4096, mask_channels=mask_c,
                                 unmasked_slots=unmasked_slots)
        g = _accumulates(masked, [lg, tg, torch.zeros(G * n), torch.zeros(8, dtype=torch.float64), mk, un], [2], [3, 5])
        cl, cu, cd = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), torch.zeros(G * n)
        K.EMU.bce_logits_groups(lg.clone(), tg.clone(), cd, cl, slots, n, 0.2, mask=mk, chw=3 * 4096, hw=4096, mask_channels=mask_c,
                                unmasked_slots=cu)
        assert rel(g["dlogit"], cd) <= 2e-5 and torch.allclose(g["loss_slots"], cl, rtol=1e-5)
        assert torch.allclose(g["unmasked_slots"], cu, rtol=1e-5)
    acc = torch.tensor([[1.0, 2.0, 3.0], [0.5, 0.0, 0.25], [7.0, 8.0, 9.0]], dtype=torch.float64)
    r = run_dirty(K.HIP, "elbo_assemble", [acc[0].clone(), acc[1].clone(), acc[2].clone(), torch.zeros(1), torch.zeros(3), 3, 4, 0.02, 1000.0],
                  [3, 4], device=DEV)
    assert_same_bits(r, what="elbo_assemble: ")
    want = (acc[0] + 1000.0 * acc[1] + 0.02 * acc[2]) / 4
    assert rel(r[ZERO]["partials"], want) < 1e-6 and abs(float(r[ZERO]["loss"]) - float(want.sum())) < 1e-3


# ---- the remaining entry points, one by one ------------------------------------------------------------------------------------
def _planes_of(src):
    """A CPU ops.Planes holding the exact three-term split of `src` ([rows][C])."""
    p = ops.Planes(src.shape[0], src.shape[1], "cpu")
    hi = src.to(torch.bfloat16)
    mid = (src - hi.float()).to(torch.bfloat16)
    p.t[:, 0], p.t[:, 1], p.t[:, 2] = hi, mid, ((src - hi.float()) - mid.float()).to(torch.bfloat16)
    return p


def _blank_planes(rows, C):
    p = ops.Planes(rows, C, "cpu")
    p.t.zero_()
    return p


def _plane_sum(t):
    f = t.float()
    return (f[:, 0] + f[:, 1]) + f[:, 2]


@pytest.mark.parametrize("G,rows,Kd,N", [(3, 37, 64, 96), (1, 130, 512, 256)])
def test_grouped_dense(G, rows, Kd, N):
    A, Bp, bias = rnd(G * rows, Kd, seed=1), rnd(G, N, Kd, seed=2, scale=0.2), rnd(G, N, seed=3)
    launch("igemm_nt_grouped", [A, Bp, bias, torch.zeros(G * rows, N), torch.zeros(G * rows, N), None, G, rows, Kd, N, 1], [3, 4],
           key=("gg", G, rows, Kd, N))
    u = rnd(G * rows, N, seed=4) * 2
    launch("igemm_nt_grouped", [A, Bp, None, torch.zeros(G * rows, N), None, u, G, rows, Kd, N, 1], [3], tol=5e-5,
           key=("ggu", G, rows, Kd, N))
    D = rnd(G * rows, N, seed=5)
    chunks = K.HIP.wgrad_chunks(DENSE, rows, N, Kd)
    launch("wgrad_tn_grouped", [D, A, torch.zeros(chunks, G, N, Kd), G, rows, N, Kd, chunks], [2], lambda i, t: t.sum(0), tol=5e-5,
           key=("gw", G, rows, Kd, N, chunks))


@pytest.mark.parametrize("G,Bg,H,dtype", [(2, 3, 32, torch.float32), (1, 2, 64, torch.float32), (4, 5, 32, torch.bfloat16)])
def test_last_decoder_layer_fused_forms(G, Bg, H, dtype, monkeypatch):
    """tconv_out3_bn_fwd / _bn_bce / _bn_bce_rows / _bn_bce_rows_grad and wgrad_out3_bn: logits, dlogit (zeros for a discarded
    pass) and the weight-gradient slabs are outputs; the loss slots and row tables are accumulators."""
    if dtype != torch.float32:
        monkeypatch.setattr(K.HIP, "precision", "bf16s")
        monkeypatch.setattr(K.EMU, "precision", "bf16s")
    rows = G * Bg * H * H
    y = (rnd(rows, 32, seed=1) * 1.5 + 0.2).to(dtype)
    mean, rstd = rnd(G, 32, seed=2) * 0.3, rnd(G, 32, seed=3).abs() + 0.5
    gamma, beta, w = rnd(32, seed=4) + 1.2, rnd(32, seed=5), rnd(32, 3, 4, 4, seed=6, scale=0.2)
    n_img = 3 * 4 * H * H
    launch("tconv_out3_bn_fwd", [y, mean, rstd, gamma, beta, w, torch.zeros(G * Bg, 3, 2 * H, 2 * H), G, Bg, H, H], [6],
           key=("o3", G, Bg, H, str(dtype)))
    target = torch.rand(Bg, 3, 2 * H, 2 * H, generator=torch.Generator().manual_seed(7))
    slots = [1, -1, 0, 2][:G] if G > 1 else [0]
    g = _accumulates("tconv_out3_bn_bce", [y, mean, rstd, gamma, beta, w, torch.zeros(Bg, 3, 2 * H, 2 * H), 0, target,
                                           torch.zeros(G * Bg * n_img), torch.zeros(4, dtype=torch.float64), slots, 0.25, G, Bg, H, H],
                     [6, 9], [10])
    cl, cd, clg = torch.zeros(4, dtype=torch.float64), torch.zeros(G * Bg * n_img), torch.zeros(Bg, 3, 2 * H, 2 * H)
    K.EMU.tconv_out3_bn_bce(y, mean, rstd, gamma, beta, w, clg, 0, target, cd, cl, slots, 0.25, G, Bg, H, H)
    assert rel(g["logits"], clg) <= 2e-5 and rel(g["dlogit"], cd) <= 2e-5 and torch.allclose(g["loss_slots"], cl, rtol=1e-5)
    if G > 1:
        assert float(g["dlogit"].view(G, -1)[1].abs().max()) == 0.0
    r = _accumulates("tconv_out3_bn_bce_rows", [y, mean, rstd, gamma, beta, w, torch.zeros(G * Bg, 3, 2 * H, 2 * H), -1, target,
                                                torch.zeros(4, Bg, dtype=torch.float64), slots, G, Bg, H, H], [6], [9])
    assert torch.allclose(r["loss_rows"].sum(1), cl, rtol=1e-5)
    w_rec = rnd(Bg, seed=8).abs() + 0.5
    rg = _accumulates("tconv_out3_bn_bce_rows_grad", [y, mean, rstd, gamma, beta, w, None, 0, target, torch.zeros(G * Bg * n_img), w_rec,
                                                      torch.zeros(4, Bg, dtype=torch.float64), slots, 0.25, G, Bg, H, H], [9], [11])
    assert torch.allclose(rg["loss_rows"].sum(1), cl, rtol=1e-5)
    want = cd.view(G, Bg, -1) * w_rec.view(1, Bg, 1)
    assert rel(rg["dlogit"].view(G, Bg, -1), want) <= 2e-5
    Gt = rnd(G * Bg, 3, 2 * H, 2 * H, seed=9)
    chunks = K.HIP.wgrad_chunks(IM2COL3, rows, 32, 64)
    launch("wgrad_out3_bn", [y, mean, rstd, gamma, beta, Gt, torch.zeros(chunks, 32, 64), G, Bg, H, chunks], [6], lambda i, t: t.sum(0),
           tol=5e-5, key=("wo3", G, Bg, H, str(dtype), chunks))


def test_row_loss_kernels():
    """The per-sample forms (elbo_loss.hip, plain and GRAD instances): row tables are accumulators (v + first == second to rtol 1e-12),
    the gradient outputs bit-identical, a discarded pass's gradient rows written as zeros; sums of the rows against the emulation's
    batch sums at the bound test_bce_logits_groups_* holds the sums to (rtol 1e-5)."""
    Bg, G, chw, hw = 5, 3, 3 * 4096, 4096
    lg, tg = rnd(G * Bg * chw, seed=400) * 3, torch.rand(Bg * chw, generator=torch.Generator().manual_seed(401))
    slots = [2, -1, 0]
    cl, cd = torch.zeros(4, dtype=torch.float64), torch.zeros(G * Bg * chw)
    K.EMU.bce_logits_groups(lg.clone(), tg.clone(), cd, cl, slots, Bg * chw, 0.2)
    r = _accumulates("bce_logits_rows_groups", [lg, tg, torch.zeros(4, Bg, dtype=torch.float64), slots, Bg, chw], [], [2])
    assert torch.allclose(r["rows_out"].sum(1), cl, rtol=1e-5)
    for mask_c in (1, 3):
        mk = (torch.rand(Bg * mask_c * hw, generator=torch.Generator().manual_seed(412)) > 0.35).float()

        def masked(be, logits, target, rows_out, mask, unmasked_rows):
            be.bce_logits_rows_groups(logits, target, rows_out, slots, Bg, chw, mask=mask, hw=hw, mask_channels=mask_c,
                                      unmasked_rows=unmasked_rows)
        rm = _accumulates(masked, [lg, tg, torch.zeros(4, Bg, dtype=torch.float64), mk, torch.zeros(4, Bg, dtype=torch.float64)], [], [2, 4])
        assert torch.allclose(rm["unmasked_rows"].sum(1), cl, rtol=1e-5)
    w_rec = rnd(Bg, seed=5).abs() + 0.5
    rg = _accumulates("bce_logits_rows_groups_grad", [lg, tg, torch.zeros(G * Bg * chw), w_rec, torch.zeros(4, Bg, dtype=torch.float64),
                                                      slots, Bg, chw, 0.2], [2], [4])
    assert rel(rg["dlogit"].view(G, Bg, chw), cd.view(G, Bg, chw) * w_rec.view(1, Bg, 1)) <= 2e-5
    assert float(rg["dlogit"].view(G, -1)[1].abs().max()) == 0.0 and torch.allclose(rg["rows_out"].sum(1), cl, rtol=1e-5)
    n = 7
    rr, tt = rnd(2 * Bg * n, seed=51), rnd(Bg * n, seed=52)
    ml, md = torch.zeros(4, dtype=torch.float64), torch.zeros(2 * Bg * n)
    K.EMU.mse_groups(rr, tt, md, ml, [1, 3], Bg * n, 0.5)
    g = _accumulates("mse_groups", [rr, tt, torch.zeros(2 * Bg * n), torch.zeros(4, dtype=torch.float64), [1, 3], Bg * n, 0.5], [2], [3])
    assert rel(g["dr"], md) < 1e-6 and torch.allclose(g["loss_slots"], ml, rtol=1e-6)
    r = _accumulates("mse_rows_groups", [rr, tt, torch.zeros(4, Bg, dtype=torch.float64), [1, 3], Bg, n], [], [2])
    assert torch.allclose(r["rows_out"].sum(1), ml, rtol=1e-6)
    rg = _accumulates("mse_rows_groups_grad", [rr, tt, torch.zeros(2 * Bg * n), w_rec, torch.zeros(4, Bg, dtype=torch.float64), [1, 3], Bg,
                                               n, 0.5], [2], [4])
    assert rel(rg["dr"].view(2, Bg, n), md.view(2, Bg, n) * w_rec.view(1, Bg, 1)) < 1e-6
    # kl_rows and the assemblies: plain outputs of fp64 tables, deterministic
    P, B, L = 3, 37, 256
    mu, lv = rnd(P, B, L, seed=60), rnd(P, B, L, seed=61)
    kr = run_dirty(K.HIP, "kl_rows", [mu, lv, torch.zeros(P, B, dtype=torch.float64), P, B, L], [2], device=DEV)
    assert_same_bits(kr, what="kl_rows: ")
    want_kl = -0.5 * (1 + lv.double() - mu.double() ** 2 - lv.double().exp()).sum(2)
    assert torch.allclose(kr[ZERO]["kl_rows"], want_kl, rtol=1e-5)
    gen = torch.Generator().manual_seed(4)
    bce, mse, kl = (torch.rand(P, B, generator=gen, dtype=torch.float64) * 100 for _ in range(3))
    kls, klw = kl.sum(1), torch.full((1,), 0.25)
    for mode in (0, 1):
        a = run_dirty(K.HIP, "elbo_assemble_rows", [bce, mse, kl, kls, torch.zeros(B), torch.zeros(P, B), P, B, 2.0, 1000.0, klw, mode],
                      [4, 5], device=DEV)
        assert_same_bits(a, what="elbo_assemble_rows: ")
        part = bce + 1000.0 * mse + 0.5 * (kl if mode else kls[:, None])
        assert torch.allclose(a[ZERO]["partials"].double(), part, rtol=1e-6) and torch.allclose(a[ZERO]["out"].double(), part.sum(0), rtol=1e-6)
        w = rnd(B, seed=7).abs() + 0.1
        aw = run_dirty(K.HIP, "elbo_assemble_weighted", [bce, mse, kl, kls, w, torch.zeros(1), torch.zeros(P), torch.zeros(B),
                                                         torch.zeros(P, B), torch.zeros(B), P, B, 2.0, 1000.0, klw, mode], [5, 6, 7, 8, 9],
                       device=DEV)
        assert_same_bits(aw, what="elbo_assemble_weighted: ")
        assert torch.equal(aw[ZERO]["out"], a[ZERO]["out"]) and torch.equal(aw[ZERO]["partials"], a[ZERO]["partials"])
        assert torch.allclose(aw[ZERO]["wpartials"].double(), (part * w.double()).sum(1) / B, rtol=1e-6)
    tab = torch.zeros(B, 4, dtype=torch.uint8)
    tab[:, 0], tab[:, 1], tab[:, 2] = torch.arange(B) % 2, torch.arange(B) % 3 != 0, torch.arange(B) % 5 != 1
    av = run_dirty(K.HIP, "elbo_assemble_rows_avail", [bce[:2].contiguous(), mse[:2].contiguous(), kl[:2].contiguous(), None, torch.zeros(B),
                                                       torch.zeros(2, B), tab, [0, 1], [2, -1], 2, B, 2.0, 1000.0, klw, 1], [4, 5],
                   state=[0, 1], device=DEV)
    assert_same_bits(av, what="elbo_assemble_rows_avail: ")
    on = tab != 0
    zb, zm = bce[:2].clone(), mse[:2].clone()
    zb[0][~on[:, 0]], zb[1][~on[:, 1]], zm[0][~on[:, 2]] = 0, 0, 0
    assert torch.equal(av[NAN]["bce_rows"], zb) and torch.equal(av[NAN]["mse_rows"], zm)
    assert torch.allclose(av[ZERO]["partials"].double(), zb + 1000.0 * zm + 0.5 * kl[:2], rtol=1e-6)


def test_availability_and_weighted_latent_kernels():
    """poe_fwd_avail / poe_bwd_avail: with every row present the results are those of poe_fwd / poe_bwd bit for bit (header); with
    a table the dmu / dlv row of an absent (row, expert) pair is WRITTEN as zeros.  poe_bwd_weighted / reparam_bwd_weighted with
    w = 1 give the unweighted kernels' gradients bit for bit (header)."""
    B, L = 37, 256
    heads = [rnd(B, 2 * L, seed=40 + i) for i in range(3)]
    dheads = [torch.zeros(B, 2 * L) for _ in range(3)]
    eps, dz = rnd(1, B, L, seed=5), rnd(1, B, L, seed=6)
    sub = [(1, 1, 1)]
    tab = torch.zeros(B, 4, dtype=torch.uint8)
    tab[:, 0], tab[:, 1], tab[:, 2] = torch.arange(B) % 2, torch.arange(B) % 3 != 0, torch.arange(B) % 5 != 1
    full = torch.ones(B, 4, dtype=torch.uint8)
    z = lambda: torch.zeros(1, B, L)

    def fwd_plain(be, h0, h1, h2, eps, mu, logvar, zz, kl_sum):
        be.poe_fwd(_passes([h0, h1, h2], [h0, h1, h2], L, sub), eps, mu, logvar, zz, kl_sum, 1, 1, B, L)

    def fwd_avail(be, h0, h1, h2, table, eps, mu, logvar, zz, kl_sum):
        be.poe_fwd_avail(_passes([h0, h1, h2], [h0, h1, h2], L, sub), [table], eps, mu, logvar, zz, kl_sum, 1, 1, B, L)
    base = run_dirty(K.HIP, fwd_plain, heads + [eps, z(), z(), z(), torch.zeros(1, dtype=torch.float64)], [4, 5, 6], state=[7], device=DEV)
    outs = {}
    for name, table in (("full", full), ("mixed", tab)):
        r = run_dirty(K.HIP, fwd_avail, heads + [table, eps, z(), z(), z(), torch.zeros(1, dtype=torch.float64)], [5, 6, 7], state=[8],
                      device=DEV)
        assert_same_bits(r, approx=("kl_sum",), what=f"poe_fwd_avail {name}: ")
        outs[name] = r[ZERO]
    for k in ("mu", "logvar", "zz"):
        assert torch.equal(outs["full"][k], base[ZERO][k]), k
    mu_a, lv_a = outs["mixed"]["mu"], outs["mixed"]["logvar"]

    def bwd_plain(be, h0, h1, h2, d0, d1, d2, eps, mu, logvar, dz):
        be.poe_bwd(_passes([h0, h1, h2], [d0, d1, d2], L, sub), eps, mu, logvar, dz, None, None, 0.02 / B, 1, 1, B, L)

    def bwd_avail(be, h0, h1, h2, d0, d1, d2, table, eps, mu, logvar, dz):
        be.poe_bwd_avail(_passes([h0, h1, h2], [d0, d1, d2], L, sub), [table], eps, mu, logvar, dz, None, None, 0.02 / B, 1, 1, B, L)

    def bwd_weighted(be, h0, h1, h2, d0, d1, d2, eps, mu, logvar, dz, w_kl):
        be.poe_bwd_weighted(_passes([h0, h1, h2], [d0, d1, d2], L, sub), eps, mu, logvar, dz, None, None, 0.02 / B, w_kl, 1, 1, B, L)
    plain = run_dirty(K.HIP, bwd_plain, heads + dheads + [eps, base[ZERO]["mu"], base[ZERO]["logvar"], dz], [3, 4, 5], device=DEV)
    assert_same_bits(plain, what="poe_bwd: ")
    fa = run_dirty(K.HIP, bwd_avail, heads + dheads + [full, eps, base[ZERO]["mu"], base[ZERO]["logvar"], dz], [3, 4, 5], device=DEV)
    assert_same_bits(fa, what="poe_bwd_avail full: ")
    wt = run_dirty(K.HIP, bwd_weighted, heads + dheads + [eps, base[ZERO]["mu"], base[ZERO]["logvar"], dz, torch.ones(B)], [3, 4, 5], device=DEV)
    assert_same_bits(wt, what="poe_bwd_weighted: ")
    ma = run_dirty(K.HIP, bwd_avail, heads + dheads + [tab, eps, mu_a, lv_a, dz], [3, 4, 5], device=DEV)
    assert_same_bits(ma, what="poe_bwd_avail mixed: ")
    for m in range(3):
        assert torch.equal(fa[ZERO][f"d{m}"], plain[ZERO][f"d{m}"]) and torch.equal(wt[ZERO][f"d{m}"], plain[ZERO][f"d{m}"]), m
        absent = tab[:, m] == 0
        assert float(ma[NAN][f"d{m}"][absent].abs().max()) == 0.0 and float(ma[NAN][f"d{m}"][~absent].abs().min()) >= 0.0

    def rb(be, h, eps, dz, d):
        be.reparam_bwd(h[:, :L], h[:, L:], eps, dz, 0.3, d[:, :L], d[:, L:], B, L, 2 * L)

    def rbw(be, h, eps, dz, w_kl, d):
        be.reparam_bwd_weighted(h[:, :L], h[:, L:], eps, dz, 0.3, w_kl, d[:, :L], d[:, L:], B, L, 2 * L)
    a = run_dirty(K.HIP, rb, [heads[0], eps[0].contiguous(), dz[0].contiguous(), torch.zeros(B, 2 * L)], [3], device=DEV)
    b = run_dirty(K.HIP, rbw, [heads[0], eps[0].contiguous(), dz[0].contiguous(), torch.ones(B), torch.zeros(B, 2 * L)], [4], device=DEV)
    assert_same_bits(b, what="reparam_bwd_weighted: ")
    assert torch.equal(a[ZERO]["d"], b[ZERO]["d"])


@pytest.mark.parametrize("B,row_len", [(37, 7), (5, 12288), (33, 10)])
def test_complete_select(B, row_len):
    g = torch.Generator().manual_seed(B * row_len)
    x, recon = torch.rand(B, row_len, generator=g), torch.rand(B, row_len, generator=g) * 60.0 - 30.0
    tab = torch.zeros(B, 4, dtype=torch.uint8)
    tab[:, 0], tab[:, 2] = torch.arange(B) % 2, torch.arange(B) % 3 != 0
    for modality in (0, 2):
        here = tab[:, modality] != 0
        for logits in (True, False):
            r = run_dirty(K.HIP, "complete_select", [x, recon, tab, modality, torch.zeros(B, row_len), logits], [4], device=DEV)
            assert_same_bits(r, what="complete_select: ")
            out = r[ZERO]["out"]
            assert torch.equal(out[here], x[here])
            if logits:      # both fp32 evaluations of 1 / (1 + exp(-x)) within 2 ulp of a result <= 1: 4 * 2^-24 (test_mixed_modal_gpu.py)
                assert float((out[~here] - torch.sigmoid(recon[~here])).abs().max()) <= 4 * 2.0 ** -24
            else:
                assert torch.equal(out[~here], recon[~here])


@pytest.mark.parametrize("rows,Kd,cd,width", [(37, 512, 3, 544), (5, 256, 10, 288), (64, 7, 4, 32)])
def test_concat_condition(rows, Kd, cd, width):
    """Every element of out is written, the zero padding included: bit-identical to torch.cat + zero padding."""
    g = torch.Generator().manual_seed(rows + Kd)
    x, cond, idx = torch.randn(rows, Kd, generator=g), torch.randn(rows, cd, generator=g), torch.randint(0, cd, (rows,), generator=g)
    for c, block in ((cond, cond), (idx, F.one_hot(idx, cd).float())):
        r = run_dirty(K.HIP, "concat_condition", [x, c, torch.zeros(rows, width), Kd, cd, torch.zeros(1, dtype=torch.int32)], [2],
                      state=[5], device=DEV)
        assert_same_bits(r, what="concat_condition: ")
        assert torch.equal(r[NAN]["out"], torch.cat((x, block, torch.zeros(rows, width - Kd - cd)), dim=-1))
        assert int(r[NAN]["bad_index"]) == 0


def test_plane_outputs_and_eval_backward(x3):
    """split_planes, the *_planes element-wise forms, dropout_reduce with `planes`, bn_eval_swish_bwd: all three planes of a plane
    output are written; hi + mid + lo is the fp32 result bit for bit."""
    G, rpg, C = 2, 700, 64
    y, da = rnd(G * rpg, C, seed=14) * 2 + 0.3, rnd(G * rpg, C, seed=15)
    mean, rstd = rnd(G, C, seed=53) * 0.2, rnd(G, C, seed=54).abs() + 0.6
    gamma, beta = rnd(C, seed=16) + 1.5, rnd(C, seed=17)
    sp = run_dirty(K.HIP, "split_planes", [y, _blank_planes(G * rpg, C)], [1], device=DEV)
    assert_same_bits(sp, what="split_planes: ")
    assert torch.equal(_plane_sum(sp[ZERO]["planes"]), y) and torch.equal(sp[ZERO]["planes"], _planes_of(y).t)
    f = launch("bn_swish_fwd", [y, mean, rstd, gamma, beta, torch.zeros(G * rpg, C), G, rpg, C, _blank_planes(G * rpg, C)], [5, 9])
    ref = emu_ref("bn_swish_fwd", [y, mean, rstd, gamma, beta, torch.zeros(G * rpg, C), G, rpg, C], [5], ("pl", G, rpg, C))[5]
    assert rel(f[ZERO]["a"], ref) <= 2e-5 and torch.equal(_plane_sum(f[ZERO]["planes"]), f[ZERO]["a"])
    only = launch("bn_swish_fwd", [y, mean, rstd, gamma, beta, None, G, rpg, C, _blank_planes(G * rpg, C)], [9])
    assert torch.equal(only[ZERO]["planes"], f[ZERO]["planes"])
    sums = rnd(G, 2, C, seed=18)
    b = launch("bn_swish_bwd_apply", [da, y, mean, rstd, gamma, beta, sums, torch.zeros(G * rpg, C), G, rpg, C, False,
                                      _blank_planes(G * rpg, C)], [7, 12])
    ref = emu_ref("bn_swish_bwd_apply", [da, y, mean, rstd, gamma, beta, sums, torch.zeros(G * rpg, C), G, rpg, C], [7], ("pl", G, rpg, C))[7]
    assert rel(b[ZERO]["dy"], ref) <= 1e-4 and torch.equal(_plane_sum(b[ZERO]["planes"]), b[ZERO]["dy"])
    masks = (torch.rand(4, 8, 512, generator=torch.Generator().manual_seed(5)) > 0.1).to(torch.uint8)
    dout, u = rnd(4, 8, 512, seed=23), rnd(8, 512, seed=52) * 2
    for extra in ([None, 0], [u, 1]):
        d = launch("dropout_reduce", [dout, masks, torch.zeros(8, 512), 4, 8, 512, 0.1] + extra + [_blank_planes(8, 512)], [2, 9])
        ref = emu_ref("dropout_reduce", [dout, masks, torch.zeros(8, 512), 4, 8, 512, 0.1] + extra, [2], ("pl", extra[1]))[2]
        assert rel(d[ZERO]["dh"], ref) <= 2e-5 and torch.equal(_plane_sum(d[ZERO]["planes"]), d[ZERO]["dh"])
    T = K.HIP.colstats_tiles(rpg)
    for da_is_du in (False, True):
        e = launch("bn_eval_swish_bwd", [da, y, mean, rstd, gamma, beta, torch.zeros(G * rpg, C), torch.zeros(G, T, 2, C), G, rpg, C,
                                         da_is_du, _blank_planes(G * rpg, C)], [6, 7, 12])
        assert torch.equal(_plane_sum(e[ZERO]["planes"]), e[ZERO]["dy"])
        # against the emulation of the two-pass form it stands in for: du and its tile sums (bound of bn_swish_bwd_reduce: 1e-4)
        if not da_is_du:
            red = emu_ref("bn_swish_bwd_reduce", [da, y, mean, rstd, gamma, beta, torch.zeros(G, 1, 2, C), G, rpg, C], [6],
                          ("ev", G, rpg, C))[6]
            assert rel(e[ZERO]["partial"].sum(1), red.sum(1)) <= 1e-4


@pytest.mark.parametrize("G,rpg,C", [(4, 700, 128), (1, 100, 256)])
def test_batchnorm_sum_forms(G, rpg, C):
    s64 = (rnd(G, 2, C, seed=3).abs() * rpg + 1.0).double()
    s64[:, 1] = s64[:, 0] ** 2 / rpg + rpg * 0.5
    rm, rv, nbt = rnd(C, seed=18), rnd(C, seed=19).abs() + 0.5, torch.zeros((), dtype=torch.long)
    fin = run_dirty(K.HIP, "bn_finalize_sums", [s64, torch.zeros(G, C), torch.zeros(G, C), rm, rv, nbt, G, C, rpg, 1e-5, 0.1, 1], [1, 2],
                    state=[3, 4, 5], device=DEV)
    assert_same_bits(fin, what="bn_finalize_sums: ")
    cpu = [s64.clone(), torch.zeros(G, C), torch.zeros(G, C), rm.clone(), rv.clone(), nbt.clone(), G, C, rpg, 1e-5, 0.1, 1]
    K.EMU.bn_finalize_sums(*cpu)
    for name, i in (("mean", 1), ("rstd", 2), ("running_mean", 3), ("running_var", 4)):
        assert rel(fin[ZERO][name], cpu[i]) < 1e-5, name
    b = rnd(G, 2, C, seed=4).double()
    launch("bn_bwd_finalize_sums", [b, torch.zeros(G, 2, C), torch.zeros(C), torch.zeros(C), G, C, 0.5, 0.0], [1, 2, 3], tol=1e-5,
           key=("bs", G, C))


@pytest.mark.parametrize("Hin,Win,Hout,Wout", [(100, 80, 80, 64), (37, 53, 20, 70)])
def test_resize_into_dirty_destination(Hin, Win, Hout, Wout):
    gen = torch.Generator().manual_seed(Hin * 1000 + Win)
    src = torch.randint(0, 256, (3, Hin, Win, 3), generator=gen, dtype=torch.uint8)
    src[1] = 255
    (xb, xk), (yb, yk) = K.EMU.resize_plan(Win, Wout, "cpu"), K.EMU.resize_plan(Hin, Hout, "cpu")
    launch("resize_u8_to_chw_f32", [src, None, torch.zeros(3, 3, Hout, Wout), 3, Hin, Win, Hout, Wout, xb, xk, yb, yk], [2], tol=0.0,
           key=("rs", Hin, Win, Hout, Wout))


@pytest.mark.parametrize("w_dtype", [torch.float32, torch.bfloat16])
def test_pack_plan_into_dirty_destinations(w_dtype, monkeypatch):
    """mmdyn_pack_plan writes every element of its destinations, the zero padding included (the product allocates them zeroed;
    nothing may depend on that): destinations pre-filled with each fill give the per-entry packs bit for bit."""
    from dirty import fill_
    from mmdyn_hip.models.shapes import image_encoder_shapes, image_decoder_shapes
    P = {}
    for k, shp in list(image_encoder_shapes("e", 256, 0, 64).items()) + list(image_decoder_shapes("d", 256, 0, 64).items()):
        if "running" in k or "num_batches" in k:
            continue
        P[k] = rnd(*shp, seed=len(P) + 7).to(DEV)
    enc = {k[2:]: v for k, v in P.items() if k.startswith("e.")}
    dec = {k[2:]: v for k, v in P.items() if k.startswith("d.")}
    specs = {"e": layers.encoder_pack_specs(enc), "h": layers.heads_pack_specs(enc), "d": layers.decoder_pack_specs(dec)}
    monkeypatch.setattr(layers, "W_DTYPE", w_dtype)
    ref = {k: layers.pack_now(v) for k, v in specs.items()}
    for fill in FILLS:
        plan = layers.PackPlan(specs, early=("W1p", "W2k", "Wf"), w_dtype=w_dtype)
        for grp in specs:
            for t in plan.packed[grp].values():
                fill_(t, fill)
        torch.cuda.synchronize()
        plan.run_early()
        plan.run_late()
        torch.cuda.synchronize()
        for grp in specs:
            for name, t in ref[grp].items():
                assert torch.equal(plan.packed[grp][name].float().cpu(), t.float().cpu()), (fill, grp, name)


# ---- the schedules: layers, scoring and serving on poisoned torch.empty memory -------------------------------------------------
def _poisoned(monkeypatch, fill):
    pt = torch if fill is None else PoisonTorch(fill)
    for mod in (ops, layers, engine):
        monkeypatch.setattr(mod, "torch", pt)


def _same_across_fills(monkeypatch, run, what, approx=()):
    """`run()` -> {name: tensor} under the real torch.empty and under each fill: every tensor bit-identical (names in `approx`:
    fp64 sums fed by atomics, rtol 1e-12)."""
    got = {}
    for fill in (None,) + FILLS:
        _poisoned(monkeypatch, fill)
        got["real torch.empty" if fill is None else fill] = {k: v.detach().cpu().clone() for k, v in run().items()}
        torch.cuda.synchronize()
    assert_same_bits(got, approx=approx, what=what)
    return got[ZERO]


def _layer_state():
    from oracle import mvae_oracle as O
    from mmdyn_hip.models.shapes import state_dict_shapes
    from mmdyn_hip.utils.seeded_init import seeded_state_dict
    return O.split_state(seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=True), 0))


def _sub(d, pre):
    return {k[len(pre) + 1:]: v.detach().clone().to(DEV) for k, v in d.items() if k.startswith(pre + ".")}


@pytest.mark.parametrize("B,G", [(4, 1), (6, 2)])
def test_layers_encoder_trunk(B, G, monkeypatch):
    """tests/test_layers_gpu.py::test_encoder_trunk's calls at its two smallest (B, G): output, every gradient and every
    BatchNorm buffer bit-identical whatever torch.empty hands out."""
    prm, buf = _layer_state()
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    dh = torch.randn(B, 512, generator=torch.Generator().manual_seed(2)).to(DEV)

    def run():
        P, Bf = _sub(prm, "visual_encoder"), _sub(buf, "visual_encoder")
        h, ctx = layers.encoder_trunk_forward(P, Bf, x, G=G)
        grads = {k: torch.zeros_like(P[k]) for k in layers.ENC_KEYS}
        layers.encoder_trunk_backward(P, ctx, dh, grads)
        out = {"h": h}
        out.update({"grad " + k: v for k, v in grads.items()})
        out.update({"buffer " + k: v for k, v in Bf.items()})
        return out
    _same_across_fills(monkeypatch, run, f"encoder trunk B={B} G={G}: ")


@pytest.mark.parametrize("B,G", [(4, 1), (8, 4)])
def test_layers_decoder(B, G, monkeypatch):
    prm, buf = _layer_state()
    z = torch.randn(B, 256, generator=torch.Generator().manual_seed(3)).to(DEV)
    dl = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)

    def run():
        P, Bf = _sub(prm, "tactile_decoder"), _sub(buf, "tactile_decoder")
        out, ctx = layers.decoder_forward(P, Bf, z, G=G)
        grads = {k: torch.zeros_like(P[k]) for k in layers.DEC_KEYS}
        dz = layers.decoder_backward(P, ctx, dl, grads)
        res = {"logits": out, "dz": dz}
        res.update({"grad " + k: v for k, v in grads.items()})
        res.update({"buffer " + k: v for k, v in Bf.items()})
        return res
    _same_across_fills(monkeypatch, run, f"decoder B={B} G={G}: ")


def test_layers_heads_and_pose_mlps(monkeypatch):
    prm, _ = _layer_state()
    gen = lambda s, *shape: torch.randn(*shape, generator=torch.Generator().manual_seed(s)).to(DEV)
    hd, dout, pose, d8, z, d10 = gen(5, 70, 512), gen(6, 70, 512), gen(7, 70, 7).abs(), gen(8, 70, 512), gen(9, 70, 256), gen(10, 70, 7)

    def run():
        res = {}
        P = _sub(prm, "visual_encoder")
        out, c = layers.heads_forward(P, hd)
        grads = {k: torch.zeros_like(P[k]) for k in layers.HEAD_KEYS}
        res.update({"heads": out, "heads dx": layers.heads_backward(c, dout, grads)})
        res.update({"heads grad " + k: v for k, v in grads.items()})
        Pe = _sub(prm, "pose_encoder")
        h2, c = layers.pose_encoder_trunk_forward(Pe, pose)
        grads = {k: torch.zeros_like(Pe[k]) for k in layers.POSE_ENC_KEYS}
        layers.pose_encoder_trunk_backward(Pe, c, d8, grads)
        res["pose h"] = h2
        res.update({"pose encoder grad " + k: v for k, v in grads.items()})
        Pp = _sub(prm, "pose_decoder")
        out, c = layers.pose_decoder_forward(Pp, z)
        grads = {k: torch.zeros_like(Pp[k]) for k in layers.POSE_DEC_KEYS}
        res.update({"pose out": out, "pose dz": layers.pose_decoder_backward(Pp, c, d10, grads)})
        res.update({"pose decoder grad " + k: v for k, v in grads.items()})
        return res
    _same_across_fills(monkeypatch, run, "heads and pose MLPs: ")


@pytest.mark.parametrize("kl", ["batch", "sample"])
def test_score_step_is_independent_of_uninitialised_memory(kl, monkeypatch):
    """MVAEStep.score_step at the smallest batch of test_model_gpu.py: rows, partials and the published reconstruction
    bit-identical; the fp64 row tables and the loss come from atomics (rtol 1e-12)."""
    from mmdyn_hip.engine import MVAEStep
    from mmdyn_hip.models import InjectedNoise
    from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise
    import test_model_emu as T
    B = 1
    inputs, targets = seeded_batch(B, 1234)
    eps, masks = seeded_noise(B, 256, 7, 8, 4321)

    def run():
        step = MVAEStep(T.build("cnn-mvae", True, True, DEV), noise=InjectedNoise(eps, masks), two_lanes=False)
        try:
            res = step.score_step([x.to(DEV) for x in inputs], [x.to(DEV) for x in targets], 0.02, kl=kl)
            torch.cuda.synchronize()
            return {k: v.double() if v.dtype == torch.float32 and k in ("loss", "loss_partials") else v
                    for k, v in res.items() if torch.is_tensor(v)}
        finally:
            step.close()
    _same_across_fills(monkeypatch, run, f"score_step kl={kl}: ",
                       approx=("rows", "partials", "bce_rows", "mse_rows", "kl_rows", "loss", "loss_partials"))


@pytest.mark.parametrize("categorical", [False, True], ids=["plain", "conditional"])
def test_serving_is_independent_of_uninitialised_memory(categorical, monkeypatch):
    """MVAEInference(use_graph=False) on the requests the serving tests make -- joint, one modality missing (not given at all, and
    absent per row through an availability table), conditional (the categorical model) -- forward, complete and score: outputs
    bit-identical; the fp64 score tables come from atomics (rtol 1e-12)."""
    import avail_cases as A
    import test_mixed_modal_emu as TM
    from mmdyn_hip.models import InjectedNoise
    inputs, eps, cond = TM.case_on(categorical, DEV, blank=0.25)
    av = A.available(3).to(DEV)

    def run():
        m, eng = TM.serving(categorical, DEV, use_graph=False)
        res = {}
        try:
            def noise():
                eng.noise = InjectedNoise([eps.clone()], [])
            requests = {"joint": dict(x=[inputs[0], inputs[1]], pose=inputs[2]), "no tactile": dict(x=[inputs[0], None], pose=inputs[2]),
                        "rows": dict(x=[inputs[0], inputs[1]], pose=inputs[2], available=av)}
            for name, rq in requests.items():
                rq = dict(rq)
                x = rq.pop("x")
                noise()
                for i, o in enumerate(eng.forward(x, condition=cond, **rq)):
                    if o is not None:
                        res[f"{name} forward {i}"] = o.clone()
            noise()
            for i, o in enumerate(eng.complete([inputs[0], inputs[1]], pose=inputs[2], available=av, condition=cond)):
                res[f"complete {i}"] = o.clone()
            noise()
            sc = eng.score([inputs[0], inputs[1]], available=av, pose=inputs[2], condition=cond, kl_weight=A.KL_WEIGHT,
                           pose_multiplier=A.POSE_MULTIPLIER)
            for k, v in sc.items():
                if torch.is_tensor(v):
                    res["score " + k] = v.clone()
                elif isinstance(v, (list, tuple)):
                    res.update({f"score {k} {i}": t.clone() for i, t in enumerate(v) if torch.is_tensor(t)})
            torch.cuda.synchronize()
        finally:
            eng.close()
        return res
    got = _same_across_fills(monkeypatch, run, "serving: ", approx=("score rows", "score kl", "score bce_visual", "score bce_tactile",
                                                                     "score mse_pose"))
    assert any(k.startswith("score ") for k in got) and "complete 2" in got


# ---- the training step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16s", "fp16s"])
def test_train_step_is_independent_of_uninitialised_memory(precision, monkeypatch):
    """MVAEStep.train_step (eager, one lane) at the smallest batch of test_model_gpu.py, identical weights and injected noise:
    with every torch.empty of ops / layers / engine pre-filled with zeros, NaNs or junk -- and with the real torch.empty -- the
    gradients, the parameters after Adam, the moments and the BatchNorm buffers are bit-identical after one step and after a
    second one (whose buffers are the first step's memory, handed back by the caching allocator).  Loss and partial ELBOs come
    from fp64 atomics: rtol 1e-12."""
    from mmdyn_hip.engine import MVAEStep
    from mmdyn_hip.models import InjectedNoise
    from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise
    import test_model_emu as T
    B = 1
    inputs, targets = seeded_batch(B, 1234)
    eps, masks = seeded_noise(B, 256, 14, 16, 4321)
    snaps = {}
    for fill in (None,) + FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else PoisonTorch(fill))
        m = T.build("cnn-mvae", True, True, DEV)
        step = MVAEStep(m, noise=InjectedNoise(eps, masks), precision=precision, two_lanes=False)
        snaps[fill] = []
        try:
            for s in range(2):
                loss = step.train_step([x.to(DEV) for x in inputs], [x.to(DEV) for x in targets], 0.02)
                torch.cuda.synchronize()
                snap = {"grad": step.params.grad, "flat": step.params.flat, "adam_m": step.adam_m, "adam_v": step.adam_v}
                snap.update({"buffer " + k: b for k, b in m.named_buffers()})
                snaps[fill].append(({k: t.detach().cpu().clone() for k, t in snap.items()},
                                    torch.cat([loss.detach().reshape(1).double().cpu(), step.partials.double().cpu()])))
        finally:
            step.close()
    for s in range(2):
        runs = {ZERO: snaps[ZERO][s][0], NAN: snaps[NAN][s][0], JUNK: snaps[JUNK][s][0], "real torch.empty": snaps[None][s][0]}
        assert_same_bits(runs, what=f"{precision}, step {s}: ")
        for fill in (None, NAN, JUNK):
            assert torch.allclose(snaps[fill][s][1], snaps[ZERO][s][1], rtol=1e-12, atol=0), (precision, s, fill)
