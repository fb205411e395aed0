"""The plane-row forms of the 3-channel layers' kernel (csrc/conv3.hip: mmdyn_conv3_fwd_planes, mmdyn_conv3_dgrad_bn_stats,
mmdyn_conv3_dgrad_bn_apply_planes) against the launches they stand in for, bit for bit:

  statistics pass  the partial-sum table == the one mmdyn_igemm_nt_dgrad_bn (which also writes du) produces;
  apply pass       the plane words == mmdyn_bn_swish_bwd_apply_planes(da_is_du = 1) fed with that launch's du and the same finalized
                   sums (the finalize of the real partial table, so the batch-mean terms are not trivial);
  forward          C == mmdyn_igemm_nt's C, the planes == mmdyn_split_planes of its C_act, for Swish and ReLU (and no activation).

The image side is 64; the sample counts are (G, Bg) = (1, 1): one sample, 8 tiles; (3, 2): groups, a grid smaller than the
persistent 1024 blocks; (2, 65): 1040 tiles -- the persistent loop's second round, its last-tile self-prefetch and a group boundary
inside the stride.  Every output is also pre-filled with NaN bit patterns and with junk: the same bits must come out."""
import ctypes

import pytest
import torch

from mmdyn_hip import ops
from mmdyn_hip.ops import IM2COL3, ACT_NONE, ACT_SWISH, ACT_RELU

pytestmark = pytest.mark.gpu

DEV = "cuda"
HIP = ops.HipBackend()
CASES = [(1, 1), (3, 2), (2, 65)]
H = 64


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)


def words(planes):
    return planes.t.view(torch.int16)


def fill(t, kind):
    """kind 0: zeros; 1: a NaN bit pattern in every word of the tensor's type; 2: junk (large finite values of both signs)."""
    raw = t.t if isinstance(t, ops.Planes) else t
    if kind == 0:
        raw.zero_()
    elif kind == 1:
        raw.view(torch.int16).fill_(0x7fc1) if raw.element_size() == 2 else raw.view(torch.int32).fill_(0x7fc00001)
    else:
        raw.copy_(((torch.arange(raw.numel(), device=raw.device) % 251).to(torch.float32) - 125.0).mul_(3.0e18).view(raw.shape))
    return t


_CACHE = {}


def problem(G, Bg):
    """Inputs and today's results for one sample count, computed once: du and the partial table of the du-writing launch, the
    finalized sums, dL/dy as planes from the stand-alone apply pass."""
    if (G, Bg) in _CACHE:
        return _CACHE[(G, Bg)]
    Bt, rows = G * Bg, G * Bg * 1024
    p = dict(G=G, Bg=Bg, rows=rows)
    p["dl"] = rnd(Bt, 3, H, H, seed=90)
    Wp = rnd(1, 32, 64, seed=91, scale=0.2)
    Wp[:, :, 48:] = 0
    p["Wp"] = Wp
    p["y"] = rnd(rows, 32, seed=92) * 1.5 + 0.2
    p["mean"], p["rstd"] = rnd(G, 32, seed=93) * 0.3, rnd(G, 32, seed=94).abs() + 0.5
    p["gamma"], p["beta"] = rnd(32, seed=95) + 1.2, rnd(32, seed=96)
    T = HIP.igemm_stat_tiles(IM2COL3, G, Bg, H, H, 64, 32, 32, 32)
    assert T == Bg * 8
    p["T"] = T
    du, partial = torch.zeros(rows, 32, device=DEV), torch.zeros(G, T, 2, 32, device=DEV)
    HIP.igemm_nt_dgrad_bn(p["dl"], Wp, du, partial, p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], IM2COL3, G, Bg, H, H, 64, 32,
                          32, 32, 1, 0)
    sums = torch.zeros(G, 2, 32, device=DEV)
    HIP.bn_bwd_finalize(partial, sums, torch.zeros(32, device=DEV), torch.zeros(32, device=DEV),
                        torch.zeros(32, G, 2, 32, device=DEV, dtype=torch.float64), G, T, 32, 0.0)
    dyp = ops.Planes(rows, 32, DEV)
    HIP.bn_swish_bwd_apply(du, p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], sums, None, G, Bg * 1024, 32, True, planes=dyp)
    torch.cuda.synchronize()
    assert float(sums.abs().min()) > 0.0 and torch.isfinite(sums).all()
    p.update(du=du, partial=partial, sums=sums, dyp=dyp)
    _CACHE[(G, Bg)] = p
    return p


@pytest.mark.parametrize("G,Bg", CASES)
def test_statistics_pass_writes_the_table_of_the_du_launch(G, Bg):
    p = problem(G, Bg)
    for kind in (0, 1, 2):
        partial = fill(torch.empty(G, p["T"], 2, 32, device=DEV), kind)
        HIP.conv3_dgrad_bn_stats(p["dl"], p["Wp"], partial, p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], G, Bg, H)
        assert not torch.isnan(partial).any(), kind
        assert torch.equal(partial, p["partial"]), (kind, float((partial - p["partial"]).abs().max()))


@pytest.mark.parametrize("G,Bg", CASES)
def test_apply_pass_writes_the_planes_of_the_stored_du_route(G, Bg):
    p = problem(G, Bg)
    for kind in (0, 1, 2):
        dyp = fill(ops.Planes(p["rows"], 32, DEV), kind)
        HIP.conv3_dgrad_bn_apply_planes(p["dl"], p["Wp"], p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], p["sums"], dyp, G, Bg, H)
        assert not torch.isnan(dyp.t.float()).any(), kind
        same = words(dyp) == words(p["dyp"])
        if not bool(same.all()):
            bad = (~same).nonzero()
            diff = float((dyp.float() - p["dyp"].float()).abs().max())
            raise AssertionError(f"fill {kind}: {bad.shape[0]} plane words differ, first at (row, plane, channel) "
                                 f"{bad[0].tolist()}, channels {sorted(set(bad[:, 2].tolist()))[:16]}, max |diff| {diff:.3e}")


@pytest.mark.parametrize("act", [ACT_SWISH, ACT_RELU, ACT_NONE])
@pytest.mark.parametrize("G,Bg", CASES)
def test_forward_writes_c_and_the_split_of_the_activated_output(G, Bg, act):
    Bt, rows = G * Bg, G * Bg * 1024
    x = rnd(Bt, 3, H, H, seed=70)
    Wp = rnd(1, 32, 64, seed=71, scale=0.2)
    Wp[:, :, 48:] = 0
    C0, Ca0 = torch.zeros(rows, 32, device=DEV), torch.zeros(rows, 32, device=DEV)
    HIP.igemm_nt(x, Wp, None, C0, Ca0, None, None, IM2COL3, 1, Bt, H, H, 64, 32, 32, 32, 32, 1, 0, act, 1)
    want = ops.Planes(rows, 32, DEV)
    HIP.split_planes(Ca0, want)
    for kind in (0, 1, 2):
        C, ap = fill(torch.empty(rows, 32, device=DEV), kind), fill(ops.Planes(rows, 32, DEV), kind)
        HIP.conv3_fwd_planes(x, Wp, C, ap, 1, Bt, H, act)
        assert not torch.isnan(C).any() and not torch.isnan(ap.t.float()).any(), kind
        assert torch.equal(C, C0), kind
        assert torch.equal(words(ap), words(want)), kind
        assert torch.equal(ap.float(), Ca0), kind            # (and the three terms add up to the fp32 activation)


def test_argument_errors_come_back_before_any_launch():
    lib, P = HIP.lib, ctypes.c_void_p
    x = torch.zeros(1, 3, H, H, device=DEV)
    Wp, C = torch.zeros(32, 64, device=DEV), torch.zeros(1024, 32, device=DEV)
    ap = fill(ops.Planes(1024, 32, DEV), 0)
    v = [torch.zeros(32, device=DEV) for _ in range(4)]
    sums, stats = torch.zeros(1, 2, 32, device=DEV), torch.zeros(1, 8, 2, 32, device=DEV)
    ptr = lambda t: P(t.data_ptr())
    fwd = [ptr(x), ptr(Wp), ptr(C), ptr(ap.t)]
    st = [ptr(x), ptr(Wp), ptr(stats), ptr(C)] + [ptr(t) for t in v]
    app = [ptr(x), ptr(Wp), ptr(C)] + [ptr(t) for t in v] + [ptr(sums), ptr(ap.t)]
    for fn, args, tail in ((lib.mmdyn_conv3_fwd_planes, fwd, (1, 1, H, ACT_SWISH)), (lib.mmdyn_conv3_dgrad_bn_stats, st, (1, 1, H)),
                           (lib.mmdyn_conv3_dgrad_bn_apply_planes, app, (1, 1, H))):
        for i in range(len(args)):                                   # every pointer is required
            a = list(args)
            a[i] = None
            assert fn(*a, *tail, None) == -2, (fn.__name__, i)
        for bad in ((0, 1, H), (1, 0, H), (1, 1, 32), (1, 1, 128), (1, 1, 65)):       # group / sample counts, image sides
            assert fn(*args, *bad, *tail[3:], None) == -1, (fn.__name__, bad)
        assert fn(*args, 1, 1 << 16, H, *tail[3:], None) == -3, fn.__name__          # rows * 32 >= 2^31
    assert lib.mmdyn_conv3_fwd_planes(*fwd, 1, 1, H, 7, None) == -1                  # an activation the kernel does not have
    torch.cuda.synchronize()
    assert float(C.abs().sum()) == 0.0 and float(stats.abs().sum()) == 0.0 and float(ap.t.float().abs().sum()) == 0.0
    # the tensor sizes the library cannot see are checked by the wrappers
    with pytest.raises(ValueError):
        HIP.conv3_fwd_planes(x, Wp, torch.zeros(1000, 32, device=DEV), ap, 1, 1, H, ACT_SWISH)
    with pytest.raises(ValueError):
        HIP.conv3_dgrad_bn_apply_planes(x, Wp, C, v[0], v[1], v[2], v[3], sums, ops.Planes(512, 32, DEV), 1, 1, H)
    with pytest.raises(ValueError):
        HIP.conv3_dgrad_bn_stats(x, Wp, torch.zeros(1, 4, 2, 32, device=DEV), C, v[0], v[1], v[2], v[3], 1, 1, H)
