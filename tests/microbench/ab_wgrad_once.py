#!/usr/bin/env python3
"""Diagnostic (LAB build): the FC-level weight gradients of the bs-256 step through the slabs (wgrad_tn / _grouped + wgrad_reduce)
against the once form (wgrad_tn_canon) on each of its tiles (MMDYN_WGRAD_ONCE_TILE) and in both block orders (MMDYN_WGRAD_ONCE_XCD),
fp32x3 (or the precision given as argv[1]); interleaved rounds after a clock warm-up, medians with min .. max, and torch.equal
against the slab result."""
import os
import statistics
import sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-dynamics_amd"))
from mmdyn_hip import ops, _lib  # noqa: E402
from mmdyn_hip.ops import DENSE  # noqa: E402

HIP = ops.HipBackend(lib_path=_lib.LAB_LIB_PATH)


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    dev = "cuda"
    arith = sys.argv[1] if len(sys.argv) > 1 else "fp32x3"
    HIP.precision, HIP.fp32_split = ("fp32", True) if arith == "fp32x3" else (arith, False)
    x = torch.randn(8192, 8192, device=dev)
    for _ in range(40):                      # ~0.3 s of matrix work: clocks up before anything is timed
        x @ x
    torch.cuda.synchronize()
    # (name, G, rows, Cd, Cg, cg_canon, perm)
    shapes = [("encoder fc_net.0", 1, 256, 512, 6400, 6400, 1), ("decoder upsample.0", 1, 1024, 6400, 256, 256, 2),
              ("heads (grouped)", 3, 1024, 512, 512, 512, 0), ("linear 512", 1, 1024, 512, 512, 512, 0)]
    for name, G, rows, Cd, Cg, cgc, perm in shapes:
        D, Gt = torch.randn(G * rows, Cd, device=dev), torch.randn(G * rows, Cg, device=dev)
        chunks = HIP.wgrad_chunks(DENSE, rows, Cd, Cg)
        assert HIP.wgrad_canon_served(rows, Cd, Cg, G)
        partial = torch.empty(chunks, G, Cd, Cg, device=dev)
        canon = {}

        def slab():
            if G == 1:
                HIP.wgrad_tn(D, Gt, partial, DENSE, rows, 1, 1, Cd, 1, 1, Cg, 1, 0, chunks)
            else:
                HIP.wgrad_tn_grouped(D, Gt, partial, G, rows, Cd, Cg, chunks)
            HIP.wgrad_reduce(partial, canon["slab"], chunks, 1, G * Cd, Cg, cgc, perm, 0.0)

        def gemm_only():
            if G == 1:
                HIP.wgrad_tn(D, Gt, partial, DENSE, rows, 1, 1, Cd, 1, 1, Cg, 1, 0, chunks)
            else:
                HIP.wgrad_tn_grouped(D, Gt, partial, G, rows, Cd, Cg, chunks)

        variants = [("slab", None, None), ("slab GEMM alone", None, None)]
        variants += [(f"once {t} xcd={o}", t, o) for t in ("128x128", "128x64", "64x64") for o in ("1", "0")]
        times = {v[0]: [] for v in variants}
        for rnd in range(7):
            for v, tile, order in variants:
                canon.setdefault(v, torch.zeros(G * Cd * cgc, device=dev))
                if tile is None:
                    fn = slab if v == "slab" else gemm_only
                else:
                    os.environ["MMDYN_WGRAD_ONCE_TILE"], os.environ["MMDYN_WGRAD_ONCE_XCD"] = tile, order
                    fn = lambda: HIP.wgrad_tn_canon(D, Gt, canon[v], G, rows, Cd, Cg, cgc, perm, 0.0, chunks)
                if rnd == 0:
                    fn()
                    torch.cuda.synchronize()
                else:
                    times[v].append(event_ms(fn, 20))
        fl = 2.0 * G * rows * Cd * Cg
        print(f"{name}: G {G} rows {rows} Cd {Cd} Cg {Cg} perm {perm} chunks {chunks} ({arith})", flush=True)
        for v, tile, _ in variants:
            t = times[v]
            m = statistics.median(t)
            same = "" if tile is None else f"  equal to slab: {torch.equal(canon[v], canon['slab'])}"
            print(f"  {v:22s} {m * 1e3:7.1f} us ({min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f})  {fl / m / 1e9:6.1f} TF/s{same}", flush=True)


if __name__ == "__main__":
    main()
