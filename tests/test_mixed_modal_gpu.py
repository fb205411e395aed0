"""Mixed-modality batches on a real MI355X: the row-available product of experts (forward, backward), the completion select and
the availability-aware assembly through the C ABI -- bit for bit against mmdyn_poe_fwd / mmdyn_poe_bwd launched with each row's
subset -- NaN isolation, guard regions; then the checks of tests/test_mixed_modal_emu.py on the HIP library and the serving
engine's replay safety.  Nothing here reads anything but the repository tree."""
import ctypes

import numpy as np
import pytest
import torch

import avail_cases as A
import test_mixed_modal_emu as TM
from mmdyn_hip import ops
from mmdyn_hip.models import InjectedNoise, NoiseSource
from test_elbo_rows_gpu import RTOL_SAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
GUARD = 256          # elements kept behind every output: they must come back untouched
MARK = 7.0

BATCHES, LATENTS = [1, 5, 37, 130, 256], [32, 256]


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(n, dtype=torch.float32, fill=float("nan")):
    """A flat device buffer of n elements + GUARD marked ones behind it."""
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    buf[n:] = MARK
    return buf


def guard_ok(buf, n):
    return bool((buf[n:] == MARK).all())


def make_heads(B, L, strided, seed):
    """Three experts: fused [B][2L] heads (mu | lv, ld = 2L) or separate dense [B][L] tensors (ld = L)."""
    g = torch.Generator().manual_seed(seed)
    if strided:
        hs = [(0.7 * torch.randn(B, 2 * L, generator=g)).to(DEV) for _ in range(3)]
        return [(h[:, :L], h[:, L:], 2 * L) for h in hs]
    return [((0.7 * torch.randn(B, L, generator=g)).to(DEV), (0.7 * torch.randn(B, L, generator=g)).to(DEV), L) for _ in range(3)]


def pass_of(heads, subset, grads=None, dz=None, zdst=None, zpl=None):
    keep = lambda m, t: t if subset[m] else None
    p = {"mu": [keep(m, h[0]) for m, h in enumerate(heads)], "lv": [keep(m, h[1]) for m, h in enumerate(heads)],
         "ld": [h[2] for h in heads]}
    if grads is not None:
        p["dmu"] = [keep(m, d[0]) for m, d in enumerate(grads)]
        p["dlv"] = [keep(m, d[1]) for m, d in enumerate(grads)]
    if dz is not None:
        p["dz"] = dz
    if zdst is not None:
        p["zdst"] = zdst
    if zpl is not None:
        p["zpl"] = zpl
    return p


def pattern(B, shift):
    """Row b holds the subset whose bits are (b + shift) % 8: every pattern, the empty one (prior alone) included."""
    code = (torch.arange(B) + shift) % 8
    return torch.stack([(code >> m) & 1 for m in range(3)] + [torch.zeros(B, dtype=torch.long)], 1).to(torch.uint8)


def fwd(heads, subset, table, eps, B, L, kl=True):
    """One forward through the C ABI (mmdyn_poe_fwd when table is the string 'old').  Returns the guarded buffers."""
    n = B * L
    mu, lv, z, zd = (guarded(n) for _ in range(4))
    zp = guarded(3 * n, torch.int16, 0)
    zp[:3 * n] = -1
    kl_sum = torch.zeros(1, dtype=torch.float64, device=DEV)
    arr = HIP._passes([pass_of(heads, subset, zdst=[zd[:n]], zpl=[None, zp.data_ptr()])])
    args = (eps.data_ptr(), mu.data_ptr(), lv.data_ptr(), z.data_ptr(), kl_sum.data_ptr() if kl else None, 1, 1, B, L, stream())
    if isinstance(table, str):
        rc = HIP.lib.mmdyn_poe_fwd(ctypes.cast(arr, ctypes.c_void_p), *args)
    else:
        tabs = (ctypes.c_void_p * 8)(None if table is None else table.data_ptr())
        rc = HIP.lib.mmdyn_poe_fwd_avail(ctypes.cast(arr, ctypes.c_void_p), ctypes.addressof(tabs), *args)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, k in ((mu, n), (lv, n), (z, n), (zd, n), (zp, 3 * n)):
        assert guard_ok(buf, k)
    return {"mu": mu[:n].view(B, L), "lv": lv[:n].view(B, L), "z": z[:n].view(B, L), "zdst": zd[:n].view(B, L),
            "zpl": zp[:3 * n].view(B, 3 * L), "kl": kl_sum}


SUBSETS8 = [tuple((c >> m) & 1 for m in range(3)) for c in range(8)]


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("L", LATENTS)
@pytest.mark.parametrize("B", BATCHES)
def test_poe_fwd_avail_bitwise(B, L, strided):
    """Every row of the new forward == the row of mmdyn_poe_fwd launched with that row's subset (mu, logvar, z, zdst, zpl), for
    every per-row subset pattern; a null table == mmdyn_poe_fwd on all rows; kl_sum against the sum of mmdyn_kl_rows."""
    heads = make_heads(B, L, strided, 100 * B + L)
    eps = torch.randn(B, L, generator=torch.Generator().manual_seed(B + L)).to(DEV)
    old = [fwd(heads, s, "old", eps, B, L) for s in SUBSETS8]
    for key in ("mu", "lv", "z", "zdst", "zpl"):
        assert torch.isfinite(old[7][key].float()).all()
    for shift in range(8 if B < 8 else 2):
        tab = pattern(B, 3 * shift)
        got = fwd(heads, (1, 1, 1), tab.to(DEV), eps, B, L)
        code = ((torch.arange(B) + 3 * shift) % 8).tolist()
        for key in ("mu", "lv", "z", "zdst", "zpl"):
            want = torch.stack([old[code[b]][key][b] for b in range(B)])
            assert torch.equal(got[key], want), (key, shift)
        rows = torch.zeros(1, B, dtype=torch.float64, device=DEV)
        HIP.kl_rows(got["mu"].contiguous(), got["lv"].contiguous(), rows, 1, B, L)
        assert torch.allclose(rows.sum(1).cpu(), got["kl"].cpu(), rtol=RTOL_SAME)
    # a pass that lacks an expert: the table cannot bring it back
    got = fwd(heads, (1, 0, 1), torch.ones(B, 4, dtype=torch.uint8, device=DEV), eps, B, L)
    assert all(torch.equal(got[k], old[5][k]) for k in ("mu", "lv", "z", "zdst", "zpl"))
    # null table (a null entry, and no array at all) == mmdyn_poe_fwd
    got = fwd(heads, (1, 1, 1), None, eps, B, L)
    assert all(torch.equal(got[k], old[7][k]) for k in ("mu", "lv", "z", "zdst", "zpl"))
    n = B * L
    mu, lv = guarded(n), guarded(n)
    arr = HIP._passes([pass_of(heads, (1, 1, 1))])
    assert HIP.lib.mmdyn_poe_fwd_avail(ctypes.cast(arr, ctypes.c_void_p), None, None, mu.data_ptr(), lv.data_ptr(), None, None, 1, 1,
                                       B, L, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(mu[:n].view(B, L), old[7]["mu"]) and torch.equal(lv[:n].view(B, L), old[7]["lv"]) and guard_ok(mu, n)


def grad_buffers(heads, B, L, strided):
    """NaN-filled gradient buffers shaped like the heads (+ guards): [(dmu, dlv)], the flat buffers."""
    if strided:
        flat = [guarded(B * 2 * L) for _ in heads]
        return [(f[:B * 2 * L].view(B, 2 * L)[:, :L], f[:B * 2 * L].view(B, 2 * L)[:, L:]) for f in flat], flat, B * 2 * L
    flat = [guarded(B * L) for _ in range(2 * len(heads))]
    return [(flat[2 * m][:B * L].view(B, L), flat[2 * m + 1][:B * L].view(B, L)) for m in range(len(heads))], flat, B * L


def bwd(heads, subset, table, eps, out, ups, B, L, strided):
    grads, flat, n = grad_buffers(heads, B, L, strided)
    dz, g_mu, g_lv, dz2, klw = ups
    arr = HIP._passes([pass_of(heads, subset, grads=grads, dz=[dz2])])
    args = (eps.data_ptr(), out["mu"].data_ptr(), out["lv"].data_ptr(), dz.data_ptr(), g_mu.data_ptr(), g_lv.data_ptr(), 0.3, 1, 1,
            B, L, klw.data_ptr(), stream())
    if isinstance(table, str):
        rc = HIP.lib.mmdyn_poe_bwd(ctypes.cast(arr, ctypes.c_void_p), *args)
    else:
        tabs = (ctypes.c_void_p * 8)(None if table is None else table.data_ptr())
        rc = HIP.lib.mmdyn_poe_bwd_avail(ctypes.cast(arr, ctypes.c_void_p), ctypes.addressof(tabs), *args)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(guard_ok(f, n) for f in flat)
    return grads


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("L", LATENTS)
@pytest.mark.parametrize("B", BATCHES)
def test_poe_bwd_avail_bitwise(B, L, strided):
    """Present (row, expert) pairs == mmdyn_poe_bwd of the row's subset, bit for bit; absent pairs are exact zeros written over
    NaN; a null table == mmdyn_poe_bwd."""
    heads = make_heads(B, L, strided, 7 * B + L)
    g = torch.Generator().manual_seed(3 * B + L)
    eps = torch.randn(B, L, generator=g).to(DEV)
    ups = [torch.randn(B, L, generator=g).to(DEV) for _ in range(4)] + [torch.full((1,), 0.5, device=DEV)]
    old_f = [fwd(heads, s, "old", eps, B, L, kl=False) for s in SUBSETS8]
    old_b = [bwd(heads, s, "old", eps, old_f[c], ups, B, L, strided) for c, s in enumerate(SUBSETS8)]
    for shift in (0, 5):
        tab = pattern(B, shift).to(DEV)
        code = ((torch.arange(B) + shift) % 8).tolist()
        out = fwd(heads, (1, 1, 1), tab, eps, B, L, kl=False)
        got = bwd(heads, (1, 1, 1), tab, eps, out, ups, B, L, strided)
        for m in range(3):
            for b in range(B):
                for k in range(2):
                    if SUBSETS8[code[b]][m]:
                        assert torch.equal(got[m][k][b], old_b[code[b]][m][k][b]), (m, b, k)
                    else:
                        assert torch.equal(got[m][k][b], torch.zeros(L, device=DEV)), (m, b, k)
    got = bwd(heads, (1, 1, 1), None, eps, old_f[7], ups, B, L, strided)
    for m in range(3):
        assert torch.equal(got[m][0], old_b[7][m][0]) and torch.equal(got[m][1], old_b[7][m][1])


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("B,L", [(5, 32), (37, 256), (130, 32)])
def test_nan_isolation(B, L, strided):
    """NaN / Inf planted in the words of every absent (row, expert): all outputs finite and bit for bit those of the clean
    heads, forward and backward."""
    clean = make_heads(B, L, strided, 11 * B + L)
    tab = pattern(B, 1)
    dirty = make_heads(B, L, strided, 11 * B + L)
    for m in range(3):
        rows = (tab[:, m] == 0).to(DEV)
        dirty[m][0][rows] = float("nan")
        dirty[m][1][rows] = float("inf") if m == 1 else float("nan")
    g = torch.Generator().manual_seed(B)
    eps = torch.randn(B, L, generator=g).to(DEV)
    ups = [torch.randn(B, L, generator=g).to(DEV) for _ in range(4)] + [torch.full((1,), 0.5, device=DEV)]
    res = []
    for heads in (clean, dirty):
        out = fwd(heads, (1, 1, 1), tab.to(DEV), eps, B, L)
        res.append((out, bwd(heads, (1, 1, 1), tab.to(DEV), eps, out, ups, B, L, strided)))
    for key in ("mu", "lv", "z", "zdst", "zpl"):
        assert torch.isfinite(res[1][0][key].float()).all() and torch.equal(res[0][0][key], res[1][0][key]), key
    assert torch.allclose(res[0][0]["kl"], res[1][0]["kl"], rtol=RTOL_SAME) and torch.isfinite(res[1][0]["kl"]).all()
    for m in range(3):
        for k in range(2):
            assert torch.isfinite(res[1][1][m][k]).all() and torch.equal(res[0][1][m][k], res[1][1][m][k])
            assert float(res[1][1][m][k][(tab[:, m] == 0).to(DEV)].abs().sum()) == 0.0


def test_argument_errors():
    lib, B, L = HIP.lib, 4, 32
    heads = make_heads(B, L, True, 1)
    arr = ctypes.cast(HIP._passes([pass_of(heads, (1, 1, 1))]), ctypes.c_void_p)
    mu, lv = torch.zeros(B, L, device=DEV), torch.zeros(B, L, device=DEV)
    tab = torch.ones(B * 4 + 4, dtype=torch.uint8, device=DEV)
    tabs = (ctypes.c_void_p * 8)(tab.data_ptr())
    odd = (ctypes.c_void_p * 8)(tab.data_ptr() + 1)
    call = lambda t, prior, P=1: lib.mmdyn_poe_fwd_avail(arr, ctypes.addressof(t), None, mu.data_ptr(), lv.data_ptr(), None, None,
                                                         prior, P, B, L, stream())
    assert call(tabs, 0) == -1                       # a table without the prior
    assert call(odd, 1) == -1                        # not word-aligned
    assert call(tabs, 1, 9) == -1
    assert lib.mmdyn_poe_fwd_avail(None, None, None, mu.data_ptr(), lv.data_ptr(), None, None, 1, 1, B, L, stream()) == -2
    assert lib.mmdyn_poe_bwd_avail(arr, ctypes.addressof(tabs), None, mu.data_ptr(), lv.data_ptr(), None, None, None, 0.0, 0, 1, B, L,
                                   None, stream()) == -1
    assert lib.mmdyn_complete_select(None, None, None, 0, mu.data_ptr(), B, L, 1, stream()) == -2
    assert lib.mmdyn_complete_select(None, mu.data_ptr(), None, 4, lv.data_ptr(), B, L, 1, stream()) == -1
    assert lib.mmdyn_elbo_assemble_rows_avail(None, None, None, None, mu.data_ptr(), None, None, None, None, 1, B, 1.0, 1.0, None, 1,
                                              stream()) == -2
    torch.cuda.synchronize()
    assert float(mu.abs().sum() + lv.abs().sum()) == 0.0                                 # nothing was launched


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("B,row_len", [(37, 7), (256, 7), (1031, 7), (5, 12288), (64, 12288), (33, 10)])
def test_complete_select(B, row_len, offset):
    """Present rows are copied bit for bit, absent rows are sigmoid(recon) (or recon itself without ``logits``); row_len 7
    (quads straddle rows, a scalar tail) and 12 288; pointers off the 16-byte grid take the element path.  Sigmoid bound: the
    largest deviation of the device's own fp32 torch.sigmoid from fp64 torch.sigmoid rounded to fp32 on the same logits (in
    [-30, 30]), times two (a different exp expansion)."""
    g = torch.Generator().manual_seed(B * row_len + offset)
    n = B * row_len
    x = torch.rand(n + offset, generator=g).to(DEV)[offset:]
    recon = ((torch.rand(n + offset, generator=g) * 60.0) - 30.0).to(DEV)[offset:]
    tab = pattern(B, 2).to(DEV)
    want_sig = torch.sigmoid(recon.double()).float()
    torch_dev = float((torch.sigmoid(recon) - want_sig).abs().max())
    for modality in (0, 2):
        present = (tab[:, modality] != 0).repeat_interleave(row_len)
        for logits in (1, 0):
            for xs in (x, None):
                buf = guarded(n + offset)
                out = buf[offset:offset + n]
                rc = HIP.lib.mmdyn_complete_select(None if xs is None else xs.data_ptr(), recon.data_ptr(), tab.data_ptr(), modality,
                                                   out.data_ptr(), B, row_len, logits, stream())
                assert rc == 0
                torch.cuda.synchronize()
                assert guard_ok(buf, n + offset)
                assert offset == 0 or bool(torch.isnan(buf[:offset]).all())
                here = present if xs is not None else torch.zeros_like(present)
                assert torch.equal(out[here], x[here])
                if logits:
                    dev_ = float((out[~here] - want_sig[~here]).abs().max()) if bool((~here).any()) else 0.0
                    print("row_len", row_len, "B", B, "kernel deviation", dev_, "torch.sigmoid deviation", torch_dev)
                    assert dev_ <= 2.0 * torch_dev
                else:
                    assert torch.equal(out[~here], recon[~here])
    # no table: every row of a given x is present; through the backend method
    out = torch.full((B, row_len), float("nan"), device=DEV)
    if offset == 0:
        HIP.complete_select(x.view(B, row_len), recon.view(B, row_len), None, 1, out, True)
        assert torch.equal(out.reshape(-1), x)


def test_assemble_rows_avail():
    """The assembly's sibling == mmdyn_elbo_assemble_rows on tables whose excluded entries were zeroed beforehand, bit for bit;
    the excluded entries (NaN planted) come back as 0."""
    B, P = 37, 2
    g = torch.Generator().manual_seed(4)
    bce, mse, kl = (torch.rand(P, B, generator=g, dtype=torch.float64) * 100 for _ in range(3))
    tab = pattern(B, 0)
    on = tab != 0
    klw = torch.full((1,), 0.25, device=DEV)
    zb, zm = bce.clone(), mse.clone()
    zb[0][~on[:, 0]], zb[1][~on[:, 1]], zm[0][~on[:, 2]] = 0, 0, 0
    want, wp = torch.empty(B, device=DEV), torch.empty(P, B, device=DEV)
    HIP.elbo_assemble_rows(zb.to(DEV), zm.to(DEV), kl.to(DEV), None, want, wp, P, B, 2.0, 1000.0, klw, 1)
    db, dm = bce.clone(), mse.clone()
    db[0][~on[:, 0]], db[1][~on[:, 1]], dm[0][~on[:, 2]] = float("nan"), float("inf"), float("nan")
    db, dm = db.to(DEV), dm.to(DEV)
    got, gp = guarded(B), guarded(P * B)
    HIP.elbo_assemble_rows_avail(db, dm, kl.to(DEV), None, got[:B], gp[:P * B], tab.to(DEV), [0, 1], [2, -1], P, B, 2.0, 1000.0, klw, 1)
    torch.cuda.synchronize()
    assert torch.equal(got[:B], want) and torch.equal(gp[:P * B].view(P, B), wp) and guard_ok(got, B) and guard_ok(gp, P * B)
    assert torch.equal(db.cpu(), zb) and torch.equal(dm.cpu(), zm)


# ---- the model layers on the HIP library -------------------------------------------------------------------------------------
@pytest.mark.parametrize("categorical", [False, True], ids=["plain", "categorical"])
def test_fixture(golden_dir, categorical):
    m, eng = TM.check_fixture(golden_dir, DEV, categorical)
    eng.close()


def test_backward():
    TM.check_backward(DEV)


def test_module_backward():
    TM.check_module_backward(DEV)


def test_interface():
    TM.check_interface(DEV)


@pytest.mark.parametrize("categorical", [False, True], ids=["plain", "categorical"])
def test_score(categorical):
    TM.check_score(DEV, categorical)


@pytest.mark.parametrize("categorical", [False, True], ids=["plain", "categorical"])
def test_complete(categorical):
    """Sigmoid bound on the device: both fp32 evaluations of 1 / (1 + exp(-x)) (the kernel's and torch's) are within 2 ulp of a
    result <= 1 (exp to 1 ulp, a correctly rounded sum and quotient), so they differ by at most 4 * 2^-24."""
    TM.check_complete(DEV, categorical, sigmoid_atol=4 * 2.0 ** -24)


def test_problem_layer():
    TM.check_problem_layer(DEV, True)


# ---- replay safety -----------------------------------------------------------------------------------------------------------
def joint_spread(eng, inputs, eps):
    """Largest difference between two eager joint forwards on identical inputs and noise, per output (0 = bitwise repeatable)."""
    runs = []
    for _ in range(2):
        eng.noise = InjectedNoise([eps.clone()], [])
        runs.append([o.clone() for o in eng.forward([inputs[0], inputs[1]], pose=inputs[2])])
    return [float((a - b).abs().max()) for a, b in zip(*runs)]


def test_joint_forward_repeatability():
    """The yardstick of the next test: is the joint forward bitwise repeatable on identical inputs?"""
    inputs, eps, _ = TM.case_on(False, DEV)
    m, eng = TM.serving(False, DEV)
    eng.use_graph = False
    spread = joint_spread(eng, inputs, eps)
    print("joint forward, two runs on identical inputs: largest differences (visual, tactile, pose, means, log_var)", spread)
    eng.close()


def test_replay_safety():
    """One captured graph, three different tables in a row: each result equals the eager run with that table; a change of the
    inputs in ABSENT rows (zeros vs a large finite constant) leaves every output row unchanged.  'Equal' / 'unchanged' is bitwise
    when the joint forward is bitwise repeatable (measured first, above and here); otherwise within that spread.  The noise-free
    outputs are compared: means / log_var of forward, and complete(sample=False)."""
    inputs, eps, _ = TM.case_on(False, DEV)
    m, eng = TM.serving(False, DEV, seed=3)
    _, eager = TM.serving(False, DEV, seed=3)
    eager.use_graph = False
    spread = joint_spread(eager, inputs, eps)
    eager.noise = NoiseSource(3)                            # (the yardstick consumed its injected draws)
    tol_img, tol_pose, tol_lat = max(spread[0], spread[1]), spread[2], max(spread[3], spread[4])
    print("repeatability spread", spread)
    same = lambda a, b, tol: float((a - b).abs().max()) <= tol and torch.isfinite(a).all()
    x = [inputs[0], inputs[1]]
    tables = [A.available(3), A.available(3).flip(0).contiguous(), 1.0 - A.available(3)]
    for tab in tables + tables[:1]:
        out = [o.clone() for o in eng.forward(x, pose=inputs[2], available=tab.to(DEV))]
        want = eager.forward(x, pose=inputs[2], available=tab.to(DEV))
        assert same(out[3], want[3], tol_lat) and same(out[4], want[4], tol_lat)
        done = [o.clone() for o in eng.complete(x, pose=inputs[2], available=tab.to(DEV))]
        want = eager.complete(x, pose=inputs[2], available=tab.to(DEV))
        assert same(done[0], want[0], tol_img) and same(done[1], want[1], tol_img) and same(done[2], want[2], tol_pose)
    assert len([k for k in eng._graphs if k[0] == "fwd"]) == 1 and len([k for k in eng._graphs if k[0] == "complete"]) == 1
    assert not torch.equal(eng.forward(x, pose=inputs[2], available=tables[0].to(DEV))[3].clone(),
                           eng.forward(x, pose=inputs[2], available=tables[2].to(DEV))[3])          # the table matters
    # absent rows' inputs: zeros vs a large finite constant
    outs = []
    for blank in (0.0, 1.0e4):
        ins, _, _ = TM.case_on(False, DEV, blank=blank)
        f = [o.clone() for o in eng.forward([ins[0], ins[1]], pose=ins[2], available=tables[0].to(DEV))]
        c = [o.clone() for o in eng.complete([ins[0], ins[1]], pose=ins[2], available=tables[0].to(DEV))]
        outs.append((f, c, ins))
    (f0, c0, i0), (f1, c1, i1) = outs
    assert same(f0[3], f1[3], tol_lat) and same(f0[4], f1[4], tol_lat)
    on = A.available(3, torch.bool).to(DEV)
    for m_ in range(3):
        tol = tol_pose if m_ == 2 else tol_img
        assert same(c0[m_][~on[:, m_]], c1[m_][~on[:, m_]], tol)                   # reconstructed rows: unchanged
        assert torch.equal(c0[m_][on[:, m_]], i0[m_][on[:, m_]])                    # present rows: the inputs
    eng.close()
    eager.close()
