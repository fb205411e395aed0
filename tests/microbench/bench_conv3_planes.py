#!/usr/bin/env python3
"""Microbenchmark of the plane-row forms of the 3-channel layers' kernel (conv3.hip) against the launches they replace, fp32
storage, 64 x 64 images, (G, Bg) = (1, 256) and (4, 256):

  last decoder layer, input gradient   old: du-writing launch + bn_swish_bwd_apply(planes, da_is_du)   new: statistics + apply pass
  first encoder layer, forward         old: forward with fp32 C_act + split_planes                      new: forward with plane rows

(the BatchNorm finalize between the two launches of a pair is the same launch either way and is left out).  Every figure is the
median of REPS timings of N launches each, with the min .. max spread of those timings beside it: a difference inside the spread
is not one.  GB/s are algorithmic bytes (every tensor once) over the time."""
import os
import statistics
import sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-dynamics_amd"))
from mmdyn_hip import ops  # noqa: E402

IM2COL3, SWISH = 3, 1
REPS, N = 7, 40


def timeit(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(N):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / N * 1e3)     # us
    return out


def line(what, ts, nbytes):
    med = statistics.median(ts)
    print(f"  {what:42s} {med:8.1f} us  ({min(ts):7.1f} .. {max(ts):7.1f})  {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e3:7.1f} GB/s", flush=True)
    return med, min(ts), max(ts)


def main():
    dev = "cuda"
    B = ops.B
    for G, Bg in ((1, 256), (4, 256)):
        Bt, rows = G * Bg, G * Bg * 1024
        print(f"(G, Bg) = ({G}, {Bg}): {rows} rows of 32 channels")
        img = torch.rand(Bt, 3, 64, 64, device=dev)
        Wp = torch.randn(1, 32, 64, device=dev) * 0.1
        Wp[:, :, 48:] = 0
        y = torch.randn(rows, 32, device=dev)
        T = B.igemm_stat_tiles(IM2COL3, G, Bg, 64, 64, 64, 32, 32, 32)
        stats, sums = torch.empty(G, T, 2, 32, device=dev), torch.randn(G, 2, 32, device=dev)
        mean, rstd = torch.randn(G, 32, device=dev) * 0.1, torch.rand(G, 32, device=dev) + 0.5
        gamma, beta = torch.rand(32, device=dev) + 0.5, torch.randn(32, device=dev) * 0.1
        du, C, Ca = (torch.empty(rows, 32, device=dev) for _ in range(3))
        planes = ops.Planes(rows, 32, dev)
        f32, pl, im = rows * 32 * 4, rows * 192, img.numel() * 4

        t_du = line("old: dgrad + BN epilogue, writes du", timeit(lambda: B.igemm_nt_dgrad_bn(
            img, Wp, du, stats, y, mean, rstd, gamma, beta, IM2COL3, G, Bg, 64, 64, 64, 32, 32, 32, 1, 0)), im + 2 * f32)
        t_ap = line("old: bn_swish_bwd_apply -> planes", timeit(lambda: B.bn_swish_bwd_apply(
            du, y, mean, rstd, gamma, beta, sums, None, G, Bg * 1024, 32, True, planes=planes)), 2 * f32 + pl)
        t_st = line("new: statistics pass (no du)", timeit(lambda: B.conv3_dgrad_bn_stats(
            img, Wp, stats, y, mean, rstd, gamma, beta, G, Bg, 64)), im + f32)
        t_a2 = line("new: apply pass -> planes", timeit(lambda: B.conv3_dgrad_bn_apply_planes(
            img, Wp, y, mean, rstd, gamma, beta, sums, planes, G, Bg, 64)), im + f32 + pl)
        old, new = t_du[0] + t_ap[0], t_st[0] + t_a2[0]
        spread = max(t[2] - t[1] for t in (t_du, t_ap, t_st, t_a2))
        print(f"  input-gradient pair: old {old:.1f} us, new {new:.1f} us, saved {old - new:.1f} us (largest spread of one timing {spread:.1f} us)")

        t_f = line("old: forward, fp32 C + C_act", timeit(lambda: B.igemm_nt(
            img, Wp, None, C, Ca, None, None, IM2COL3, G, Bg, 64, 64, 64, 32, 32, 32, 32, 1, 0, SWISH, 1)), im + 2 * f32)
        t_s = line("old: split_planes", timeit(lambda: B.split_planes(Ca, planes)), f32 + pl)
        t_n = line("new: forward, fp32 C + plane rows", timeit(lambda: B.conv3_fwd_planes(img, Wp, C, planes, G, Bg, 64, SWISH)),
                   im + f32 + pl)
        old, new = t_f[0] + t_s[0], t_n[0]
        spread = max(t[2] - t[1] for t in (t_f, t_s, t_n))
        print(f"  forward: old {old:.1f} us, new {new:.1f} us, saved {old - new:.1f} us (largest spread of one timing {spread:.1f} us)")


if __name__ == "__main__":
    main()
