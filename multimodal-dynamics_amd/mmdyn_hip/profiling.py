"""Per-kernel timing with HIP events on the launch stream (bench.py's ``roofline`` object).

``TimedBackend`` wraps the active backend: every kernel-launching call is bracketed by two events recorded
on torch's current stream -- the stream the C ABI launches on -- and tagged with its algorithmic FLOPs /
bytes, so achieved rates are measured live rather than taken from a trace."""
import collections

import torch

from . import ops

PAD_CYCLES = 100000       # torch.cuda._sleep argument: ~43 us on an MI355X
HOST_ONLY = {"igemm_stat_tiles", "colstats_tiles", "wgrad_chunks", "igemm_planes_served", "wgrad_canon_served"}


def _canon(name, a):
    """The dgrad+BatchNorm-backward launch is the same kernel family: book it as igemm_nt with igemm_nt's argument
    order (A, Bp, bias, C, C_act, stats, ws, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, ldc, stride, offset, act, splitk)."""
    if name == "igemm_nt_dgrad_bn":
        A, Bp, C, stats, y, mean, rstd, gamma, beta, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride, offset = a
        name, a = "igemm_nt", (A, Bp, y, C, None, stats, None, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, N, stride, offset, 0, 1)
    if name == "igemm_nt_dgrad_act":      # ... and the dgrad + activation-backward launch
        A, Bp, C, u, act, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride, offset = a
        name, a = "igemm_nt", (A, Bp, u, C, None, None, None, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, N, stride, offset, 0, 1)
    if name == "igemm_nt_grouped":        # G dense GEMMs of one shape in one launch: the same kernels, G groups of `rows` rows
        A, Bp, bias, C, C_act, u, G, rows, K, N, act = a
        name, a = "igemm_nt", (A, Bp, bias if u is None else u, C, C_act, None, None, ops.DENSE, G, rows, 1, 1, K, 1, 1, N, N, 1, 0, act, 1)
    if name == "wgrad_tn_grouped":
        D, Gt, partial, G, rows, Cd, Cg, chunks = a
        name, a = "wgrad_tn", (D, Gt, partial, ops.DENSE, G * rows, 1, 1, Cd, 1, 1, Cg, 1, 0, chunks)
    if name == "wgrad_tn_canon":          # the once form of wgrad_tn_kernel: the same GEMM (and FLOPs), canon in place of the slabs
        D, Gt, canon, G, rows, Cd, Cg, cg_canon, perm, beta, chunks = a
        name, a = "wgrad_tn", (D, Gt, canon, ops.DENSE, G * rows, 1, 1, Cd, 1, 1, Cg, 1, 0, chunks)
    if name == "wgrad_out3_bn":          # the last decoder layer's weight gradient with the fused BatchNorm + Swish (conv3_wgrad_kernel)
        y, mean, rstd, gamma, beta, Gt, partial, G, Bg, Hr, chunks = a
        return "conv3_wgrad", (y, Gt, partial, ops.IM2COL3, G * Bg, Hr, Hr, 32, 2 * Hr, 2 * Hr, 64, 1, 0, chunks)
    if name == "tconv_out3_bn_fwd":
        return "tconv_out3_fwd", a
    # the plane-row forms of conv3_nt_kernel: the same main loop (and FLOPs) as the launches they stand in for
    if name == "conv3_fwd_planes":
        x, Wp, C, planes, G, Bg, H, act = a
        return "conv3_nt", (x, Wp, None, C, planes, None, None, ops.IM2COL3, G, Bg, H, H, 64, H // 2, H // 2, 32, 32, 1, 0, act, 1)
    if name == "conv3_dgrad_bn_stats":
        x, Wp, stats, y, mean, rstd, gamma, beta, G, Bg, H = a
        return "conv3_nt", (x, Wp, y, None, None, stats, None, ops.IM2COL3, G, Bg, H, H, 64, H // 2, H // 2, 32, 32, 1, 0, 0, 1)
    if name == "conv3_dgrad_bn_apply_planes":
        x, Wp, y, mean, rstd, gamma, beta, sums, planes, G, Bg, H = a
        return "conv3_nt", (x, Wp, y, planes, None, None, None, ops.IM2COL3, G, Bg, H, H, 64, H // 2, H // 2, 32, 32, 1, 0, 0, 1)
    # the 3-channel layers run their own kernels (csrc/conv3.hip), not igemm_nt_kernel / wgrad_tn_kernel: booked apart so
    # that the launch counts and average durations of the MFMA families match what rocprofv3 reports per kernel name
    if name == "igemm_nt" and a[7] == ops.IM2COL3 and a[10] in (64, 128, 256) and \
            tuple(a[10:17]) == (a[10], a[10], 64, a[10] // 2, a[10] // 2, 32, 32):
        return "conv3_nt", a
    # ... and so does the 64 -> 32 channel transposed convolution on 16x16 inputs in fp32 (csrc/tconv_patch.hip)
    if name == "igemm_nt" and a[7] == ops.TCONV_S2P1 and tuple(a[10:16]) in ((16, 16, 64, 32, 32, 32), (32, 32, 32, 64, 64, 32),
                                                                            (64, 64, 32, 128, 128, 32)) and \
            getattr(ops.B, "precision", "fp32") == "fp32" and all(not torch.is_tensor(t) or t.dtype == torch.float32 for t in a[:4]):
        return "tconv_patch", a
    if name == "wgrad_tn" and a[3] == ops.IM2COL3 and a[8] in (64, 128, 256) and \
            tuple(a[5:11]) == (a[8] // 2, a[8] // 2, 32, a[8], a[8], 64):
        return "conv3_wgrad", a
    return name, a


def _flops(name, a):
    if name in ("igemm_nt", "conv3_nt", "tconv_patch"):
        (mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N) = a[7:16]
        if mode == ops.DENSE:
            return 2.0 * G * Bg * Ho * Wo * N * Cin
        if mode == ops.CONV:
            return 2.0 * G * Bg * Ho * Wo * N * 16 * Cin
        if mode == ops.TCONV_S1P0:
            return 2.0 * G * Bg * Hi * Wi * N * 16 * Cin
        if mode == ops.IM2COL3:
            return 2.0 * G * Bg * Ho * Wo * N * 48
        return 2.0 * G * Bg * Ho * Wo * N * 4 * Cin
    if name in ("wgrad_tn", "conv3_wgrad"):
        (mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg) = a[3:11]
        return 2.0 * Bt * Hr * Wr * Cd * Cg * (16 if mode == ops.CONV else 1)
    return 0.0


def _bytes(a):
    n = 0
    for t in a:
        if isinstance(t, ops.Planes):
            t = t.t
        if torch.is_tensor(t):
            n += t.numel() * t.element_size()
    return n


class TimedBackend:
    name = "hip"

    def __init__(self, inner):
        self._inner = inner
        self.records = []

    @property
    def precision(self):
        return self._inner.precision

    @precision.setter
    def precision(self, value):
        self._inner.precision = value

    @property
    def fp32_split(self):
        return getattr(self._inner, "fp32_split", False)

    @fp32_split.setter
    def fp32_split(self, value):
        self._inner.fp32_split = value

    def __getattr__(self, attr):
        fn = getattr(self._inner, attr)
        if attr in HOST_ONLY or not callable(fn):
            return fn

        def wrapped(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            # A ~40 us spin kernel (one wave, no memory traffic) in front of the start event: the GPU reaches the event only after the
            # host has queued the launch and the end event behind it, so the bracket holds the kernel(s) of the call and not the host's
            # launch latency -- which an eager pass otherwise books on every kernel shorter than it (the FC-level GEMMs read 33-36 us by
            # events against 13-22 us in the rocprofv3 trace of the same run).
            torch.cuda._sleep(PAD_CYCLES)
            s.record()
            r = fn(*a, **k)
            e.record()
            name, ca = _canon(attr, a)
            sig = tuple(x for x in ca if isinstance(x, (int, bool))) if name in ("igemm_nt", "wgrad_tn", "conv3_nt", "conv3_wgrad", "tconv_patch") else ()
            if attr == "igemm_nt_dgrad_bn":
                sig = sig + ("bn_bwd_epilogue",)
            if attr == "igemm_nt_dgrad_act":
                sig = sig + ("act_bwd_epilogue",)
            if attr in ("igemm_nt_grouped", "wgrad_tn_grouped"):
                sig = sig + ("grouped",)
            self.records.append((name, _flops(name, ca), _bytes(ca), s, e, sig))
            return r
        return wrapped

    def summary(self):
        torch.cuda.synchronize()
        agg = collections.OrderedDict()
        self.by_shape = collections.OrderedDict()
        for name, fl, by, s, e, sig in self.records:
            if sig:
                d2 = self.by_shape.setdefault((name,) + sig, {"calls": 0, "ms": 0.0, "flops": 0.0})
                d2["calls"] += 1
                d2["ms"] += s.elapsed_time(e)
                d2["flops"] += fl
            d = agg.setdefault(name, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["calls"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += fl
            d["bytes"] += by
        return agg


def profile_step(fn):
    """Run ``fn()`` once with every kernel call timed; returns {kernel: {calls, ms, flops, bytes}}."""
    timed = TimedBackend(ops.B)
    old = ops.set_backend(timed)
    try:
        fn()
    finally:
        ops.set_backend(old)
    out = timed.summary()
    profile_step.by_shape = timed.by_shape
    return out
