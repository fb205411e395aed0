#!/usr/bin/env python3
"""What one grid of the epoch image log costs on one GPU, at the workload's shape: two tensors of 256 decoder logits 3 x 64 x 64,
take = 120, nrow = 16 (240 tiles, a 992 x 1058 canvas).  (1) mmdyn_image_grid_u8: one launch, uint8 HWC out.  (2) The same grid from
stock torch ops as the reference builds it (problems.py:565, 599-603): sigmoid of both whole batches, two slices, torch.cat, a zero
canvas and one copy_ per tile (torchvision.utils.make_grid's loop, restated here: torchvision is not a dependency), then the
writer's * 255 -> clip -> uint8 on the device (the reference does that on the host, after an fp32 copy of the canvas).  The two
alternate, windows of `reps` calls between device events; the bytes over the kernel's time are the bytes the algorithm needs
(240 tiles read once, the canvas written once).  Both results are compared before anything is timed."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-dynamics_amd"))
from mmdyn_hip import ops  # noqa: E402

DEV = "cuda"
N_IMG, TAKE, NROW, PAD, S = 256, 120, 16, 2, 64


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_grid(a, b):
    img = torch.cat((torch.sigmoid(a)[:TAKE], torch.sigmoid(b)[:TAKE]), 0)
    n = img.shape[0]
    xmaps = min(NROW, n)
    ymaps = -(-n // xmaps)
    h, w = S + PAD, S + PAD
    grid = img.new_zeros((3, h * ymaps + PAD, w * xmaps + PAD))
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            grid.narrow(1, y * h + PAD, S).narrow(2, x * w + PAD, S).copy_(img[k])
            k += 1
    return (grid * 255).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def main(rounds=9, reps=50):
    torch.manual_seed(0)
    a, b = (3 * torch.randn(N_IMG, 3, S, S, device=DEV) for _ in range(2))
    out = torch.empty(ops.grid_shape(2 * TAKE, S, S, NROW, PAD) + (3,), dtype=torch.uint8, device=DEV)
    ours = lambda: ops.B.image_grid([a, b], TAKE, NROW, True, PAD, out=out)
    theirs = lambda: torch_grid(a, b)
    diff = (ours().int() - theirs().int()).abs()
    print(f"grid {tuple(out.shape)}: bytes that differ from the torch-op grid {int((diff != 0).sum())} of {out.numel()}, "
          f"largest difference {int(diff.max())}", flush=True)
    assert int(diff.max()) <= 1 and int((diff != 0).sum()) <= out.numel() // 100
    x = torch.randn(8192, 8192, device=DEV)
    for _ in range(40):                      # clocks up before anything is timed
        x @ x
    for fn in (ours, theirs):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(rounds):
        t_ours.append(event_ms(ours, reps))
        t_theirs.append(event_ms(theirs, reps))
    need = 2 * TAKE * 3 * S * S * 4 + out.numel()
    for name, t in (("mmdyn_image_grid_u8 (1 launch)", t_ours), ("torch ops (sigmoid x 2, cat, zeros, 240 copy_, * 255, clamp, to, permute)", t_theirs)):
        med = statistics.median(t)
        print(f"  {name:76s} {med * 1e3:9.2f} us  ({min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f})"
              + (f"  {need / med / 1e9:.3f} TB/s of the {need / 1e6:.1f} MB it needs" if t is t_ours else ""), flush=True)


if __name__ == "__main__":
    main()
