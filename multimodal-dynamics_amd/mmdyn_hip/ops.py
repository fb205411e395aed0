"""Tensor-level wrappers over the C ABI (include/mmdyn_hip.h).

Every method of :class:`HipBackend` maps 1:1 onto one ``mmdyn_*`` entry point: it validates device /
dtype / contiguity, passes raw device pointers and launches on torch's *current* HIP stream.  PyTorch is
used only for memory, streams and autograd plumbing -- all arithmetic of the hot path happens in
libmmdyn_hip.so.  There is no CPU / ATen fallback: a CPU tensor raises.

``B`` is the active backend.  The test-suite may swap in an emulation object (tests/emu_backend.py) to
exercise the host-side orchestration on a machine without a GPU; nothing in the product does.
"""
import ctypes
import numbers

import os

import torch

from . import _lib
from ._lib import PassExperts, FeedGroups, GatherGroups, EnsembleGroups, QuantileGroups, MAX_PASSES, MAX_EXPERTS, FEED_GROUPS, check

ACT_NONE, ACT_SWISH, ACT_RELU = 0, 1, 2
DENSE, CONV, TCONV_S2P1, IM2COL3, TCONV_S1P0 = 0, 1, 2, 3, 4
ROW_GROUPS_MAX = 8         # MMDYN_BCE_GROUPS_MAX: the passes one launch of a *_groups kernel walks over its target
PLAN_TOP_MAX = 8           # MMDYN_PLAN_TOP_MAX: the longest list of best candidates mmdyn_plan_select_steps keeps per row
REFIT_N_MAX = 4096         # MMDYN_REFIT_N_MAX: the candidates per row whose cost column mmdyn_plan_refit ranks in LDS
QUANTILES_MAX = 8          # MMDYN_QUANTILES_MAX: the order statistics one mmdyn_ensemble_quantiles launch forms per element
QUANTILE_N_MAX = 128       # MMDYN_QUANTILE_N_MAX: the samples per element that launch ranks in LDS


def _ptr(t, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("mmdyn_hip: the HIP path needs GPU tensors (got a CPU tensor); there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"mmdyn_hip: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("mmdyn_hip: tensor must be contiguous")
    return t.data_ptr()


def _aptr(t):
    """Pointer of an ACTIVATION (or packed-weight) tensor: fp32, or 16-bit in the storage modes.  Returns (pointer, fmt):
    fmt 0 = fp32, 1 = bf16 ("bf16s"), 2 = IEEE half ("fp16s") -- truthy exactly for the 16-bit formats."""
    if t is None:
        return None, 0
    if t.dtype == torch.bfloat16:
        return _ptr(t, torch.bfloat16), 1
    if t.dtype == torch.float16:
        return _ptr(t, torch.float16), 2
    return _ptr(t), 0


def _is16(t):
    return t.dtype in (torch.bfloat16, torch.float16)


def _half(*fmts):
    """1 when the 16-bit tensors of one call are IEEE half, 0 when bf16 (or none); the two never mix in one call."""
    kinds = {f for f in fmts if f}
    if len(kinds) > 1:
        raise TypeError("mmdyn_hip: bf16 and fp16 tensors in one call")
    return int(2 in kinds)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_clip(clip, name):
    if not torch.is_tensor(clip) or clip.dtype != torch.float64 or clip.numel() != 4 or not clip.is_contiguous():
        raise ValueError(f"mmdyn_{name}: clip must be four contiguous fp64 values {{sum of squares, norm, coefficient, clipped steps}}")


def check_max_norm(value, what):
    """``value`` as a float if it is a real number > 0 (inf allowed: report the norm, never clip), else a ValueError naming ``what``."""
    if not (isinstance(value, numbers.Real) and not isinstance(value, bool) and float(value) > 0.0):
        raise ValueError(f"{what} must be a real number > 0 (inf: report the gradient norm without clipping), got {value!r}")
    return float(value)


def check_ema_decay(value, what):
    """``value`` as a float if it is a real number in [0, 1), else a ValueError naming ``what``."""
    if not (isinstance(value, numbers.Real) and not isinstance(value, bool) and 0.0 <= float(value) < 1.0):
        raise ValueError(f"{what} must be a real number in [0, 1), got {value!r}")
    return float(value)


def new_ema_state(decay, warmup, device):
    """The EMA state of include/mmdyn_hip.h on ``device``: fp64 {updates done = 0, decay, 1 - d_n = 0, warm-up flag}."""
    decay = check_ema_decay(decay, "ema_decay")
    return torch.tensor([0.0, decay, 0.0, 1.0 if warmup else 0.0], dtype=torch.float64).to(device)


def _check_ema(ema, p, ema_state, name):
    if not torch.is_tensor(ema_state) or ema_state.dtype != torch.float64 or ema_state.numel() != 4 or not ema_state.is_contiguous():
        raise ValueError(f"mmdyn_{name}: ema_state must be four contiguous fp64 values {{updates, decay, 1 - d_n, warm-up flag}}")
    if ema is None:
        return
    if not torch.is_tensor(ema) or not torch.is_tensor(p) or ema.numel() != p.numel():
        raise ValueError(f"mmdyn_{name}: ema must hold as many elements as p")
    n = p.numel() * p.element_size()
    if ema.device == p.device and ema.data_ptr() < p.data_ptr() + n and p.data_ptr() < ema.data_ptr() + n:
        raise ValueError(f"mmdyn_{name}: ema must not alias p")


def grid_shape(N, H, W, nrow, padding=2):
    """(Hg, Wg) of ``torchvision.utils.make_grid`` on N images of H x W: xmaps = min(nrow, N) tiles per row, ceil(N / xmaps) rows,
    ``padding`` pixels around every tile; a single image comes back alone.  Host arithmetic of mmdyn_image_grid_u8."""
    N, H, W, nrow, padding = int(N), int(H), int(W), int(nrow), int(padding)
    if N < 1 or H < 1 or W < 1 or nrow < 1 or padding < 0:
        raise ValueError(f"grid_shape: N, H, W, nrow >= 1 and padding >= 0, got {(N, H, W, nrow, padding)}")
    if N == 1:
        return H, W
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def check_grid_sources(srcs, take, nrow, padding):
    """The one or two sources of ``image_grid`` as a list, after the checks that need no device: fp32, contiguous, 4-D, C in {1, 3},
    one C / H / W, one device; ``take`` / ``nrow`` >= 1, ``padding`` >= 0.  A ValueError names what is wrong."""
    srcs = [srcs] if torch.is_tensor(srcs) else srcs
    if not isinstance(srcs, (list, tuple)) or not 1 <= len(srcs) <= 2 or not all(torch.is_tensor(s) for s in srcs):
        raise ValueError("mmdyn_image_grid_u8: srcs is a tensor, or a list / tuple of one or two tensors")
    for s in srcs:
        if s.dtype != torch.float32 or s.dim() != 4 or not s.is_contiguous() or s.shape[0] < 1 or s.shape[1] not in (1, 3):
            raise ValueError(f"mmdyn_image_grid_u8: a source is contiguous fp32 [n >= 1][C in (1, 3)][H][W], got {s.dtype} "
                             f"{tuple(s.shape)}{'' if s.is_contiguous() else ' (not contiguous)'}")
        if s.shape[1:] != srcs[0].shape[1:] or s.device != srcs[0].device:
            raise ValueError(f"mmdyn_image_grid_u8: the sources differ in C / H / W or device: {tuple(srcs[0].shape)} on "
                             f"{srcs[0].device}, {tuple(s.shape)} on {s.device}")
    for what, v, low in (("take", take, 1), ("nrow", nrow, 1), ("padding", padding, 0)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < low:
            raise ValueError(f"mmdyn_image_grid_u8: {what} must be an integer >= {low}, got {v!r}")
    return list(srcs)


def check_grid_out(out, shape, device):
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() \
            or out.device != device:
        raise ValueError(f"mmdyn_image_grid_u8: out must be a contiguous uint8 tensor {shape} on {device}")


class Planes:
    """An fp32 matrix [rows][C] kept as its exact three-term bf16 split, the operand format of the fp32x3 GEMMs that take their
    operands ALREADY SPLIT (include/mmdyn_hip.h, flag bits 7 + 8): ``t[row][plane][c]`` (torch.bfloat16), plane 0 = hi = bf16(x),
    1 = mid = bf16(x - hi), 2 = lo = x - hi - mid; hi + mid + lo == x bit for bit.  Written by ``B.split_planes`` (or by the
    kernels that produce the tensor); a channels-last activation has one row per pixel, packed weights one per (tap, n)."""
    __slots__ = ("t",)

    def __init__(self, rows, C, device):
        if C % 8:
            raise ValueError("mmdyn_hip: plane rows are moved in 8-channel granules (C % 8 == 0)")
        self.t = torch.empty(rows, 3, C, dtype=torch.bfloat16, device=device)

    @property
    def rows(self):
        return self.t.shape[0]

    @property
    def C(self):
        return self.t.shape[2]

    def float(self):
        """The fp32 matrix back (exact: hi + mid has at most 16 significant bits, + lo is x)."""
        f = self.t.to(torch.float32)
        return (f[:, 0] + f[:, 1]) + f[:, 2]


# The "last block finishes" single-launch forms of mmdyn_bn_finalize / mmdyn_bn_bwd_finalize / mmdyn_colsum are not taken by
# EVERY launch: measured on the two-lane step that cost 0.12 ms (fp32 bs 256: 6.78 -> 6.90 ms; bf16s bs 128: 2.165 -> 2.19 ms) --
# up to 1024 blocks arrive on one counter (~12 ns per arrival) and every block drains its stores before it may leave
# (docs/LAB_NOTES.md D).  The BatchNorm finalize launches with SMALL partial tables take it (HipBackend.ticket_max_work, round 6:
# LAB_NOTES H.g); MMDYN_TICKET=1 switches it on everywhere (kernel tests, experiments).
_USE_TICKET = bool(os.environ.get("MMDYN_TICKET"))


class HipBackend:
    name = "hip"

    def __init__(self, lib_path=None):
        self._l, self._lib_path = None, lib_path       # lib_path: the LAB build (tests / microbenchmarks only)
        self._tickets = {}                             # device -> [zeroed int32 pool, next eager slot, next graph slot, free graph slots]
        self._drawn = None                             # (device, slot) pairs drawn by captured launches since ticket_mark()
        self.use_flags = False                         # (the product library ignores arrival words: see _flags)
        self._flagpool = {}                            # device -> [zeroed int32 pool, next eager block, next graph block, free graph blocks]
        self.force_ticket = False
        # BatchNorm finalize launches whose partial-sum table has at most this many (group, tile) rows take the single-launch
        # "last block finishes" form (0: none, rounds 3-5 -- the form lost on the whole step when EVERY finalize took it).  Same
        # box, interleaved (profiles/r6/ab_bn_finalize_small_tables.txt, bench.py --ticket-max-work): 1024 = nothing on the
        # power-bound configs[1] step, +1.1 % on bf16s bs 128, 18 launches fewer per step; bit-identical results either way (a table
        # of 640 tiles or more per group runs as two launches inside the library even with a ticket: csrc/bn.hip)
        self.ticket_max_work = 1024
        # "fp32": v_mfma_f32_32x32x2_f32 (the reference's arithmetic, the default and the BASELINE configs[1] path);
        # "bf16": operands rounded to bf16 on their way into the matrix cores, fp32 accumulate (configs[2]);
        # "fp16": the same with IEEE-half operands (configs[4]); "bf16s": bf16 + bf16 activation storage;
        # "fp16s": fp16 + fp16 activation storage
        self.precision = "fp32"
        # With precision "fp32": let the fp32 GEMM launches that gain from it run on the bf16 matrix cores through the EXACT
        # three-term split of their fp32 operands (x = hi + mid + lo, six of nine products, fp32 accumulate: csrc/igemm_nt.hip
        # X3; error against fp64 no larger than the native fp32 matrix cores').  The engines' precision "fp32x3" sets it.
        self.fp32_split = False

    TICKET_SLOTS, TICKET_STRIDE = 4096, 16             # one 64-byte line per slot

    def _ticket(self, like, work=None):
        """Address of a zero-initialised arrival counter for ONE launch (the "last block finishes" kernels:
        mmdyn_bn_finalize, mmdyn_bn_bwd_finalize, mmdyn_colsum); the kernel that used a slot leaves it zero.
        A launch recorded into a HIP graph keeps its slot for every replay, so captured launches draw from the lower half
        of the pool, and a slot handed out there belongs to that graph until its owner gives it back: the engines bracket a
        capture with ticket_mark() / ticket_take() and call ticket_release() with the slots of a graph they drop (a
        recapture on a new batch shape), so a long run that recaptures every epoch does not run out.  Eager
        launches cycle through the upper half: a slot comes up again only after 2048 eager launches of this kind -- far more
        than a train step issues -- so no two launches in flight share one, and none can meet a slot that a replaying graph
        owns."""
        if not (_USE_TICKET or self.force_ticket or (work is not None and work <= self.ticket_max_work)):
            return None
        dev = like.device
        ent = self._tickets.get(dev)
        if ent is None:
            ent = [torch.zeros(self.TICKET_SLOTS * self.TICKET_STRIDE, dtype=torch.int32, device=dev), 0, 0, []]
            self._tickets[dev] = ent
        pool, nxt_eager, nxt_graph, free = ent
        half = self.TICKET_SLOTS // 2
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            if free:
                slot = free.pop()
            elif nxt_graph >= half:
                raise RuntimeError("mmdyn_hip: ticket slots for captured launches exhausted (2048 live per device)")
            else:
                ent[2] = nxt_graph + 1
                slot = nxt_graph
            if self._drawn is not None:
                self._drawn.append((dev, slot))
        else:
            ent[1] = (nxt_eager + 1) % half
            slot = half + nxt_eager
        return pool.data_ptr() + 4 * self.TICKET_STRIDE * slot

    # arrival words of the persistent stream-K GEMMs (igemm_wsp.hip, round 6): one block of FLAG_WORDS zeroed words per launch, the
    # same ownership rules as the tickets (captured launches own theirs until ticket_release, eager launches cycle through the upper
    # half); the kernel leaves every word it set back at zero.  Exhausted (hundreds of live captures): None -- the launch then takes
    # the two-launch form (slabs + fix-up kernel).  ``use_flags`` is False by default: finishing split tiles inside the launch is
    # built, tested bit-identical and measured SLOWER on the step (docs/LAB_NOTES.md H.a); the product library compiles it out and
    # only the LAB library honours the words (tests, bench.py --inkernel-finish with MMDYN_HIP_LIB pointing at the LAB build).
    FLAG_BLOCKS, FLAG_WORDS = 1024, 8192

    def _flags(self, like):
        if not self.use_flags:       # (A/B measurements and the bit-equality test against the two-launch form)
            return None
        dev = like.device
        ent = self._flagpool.get(dev)
        if ent is None:
            ent = [torch.zeros(self.FLAG_BLOCKS * self.FLAG_WORDS, dtype=torch.int32, device=dev), 0, 0, []]
            self._flagpool[dev] = ent
        pool, nxt_eager, nxt_graph, free = ent
        half = self.FLAG_BLOCKS // 2
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            if free:
                blk = free.pop()
            elif nxt_graph >= half:
                return None
            else:
                ent[2] = nxt_graph + 1
                blk = nxt_graph
            if self._drawn is not None:
                self._drawn.append((dev, -1 - blk))            # (negative: a flag block, not a ticket slot)
        else:
            ent[1] = (nxt_eager + 1) % half
            blk = half + nxt_eager
        return pool.data_ptr() + 4 * self.FLAG_WORDS * blk

    def ticket_mark(self):
        """Start recording the slots that captured launches draw (one capture at a time)."""
        self._drawn = []

    def ticket_take(self):
        """The slots drawn since ticket_mark(): they belong to the graph(s) just captured."""
        drawn, self._drawn = self._drawn or [], None
        return drawn

    def ticket_release(self, slots):
        """Give back the slots of graphs that will never be replayed again.  The caller has synchronised the device (a replay
        still in flight would otherwise share its counter with the next capture's launch)."""
        for dev, slot in slots or ():
            if slot < 0:
                self._flagpool[dev][3].append(-1 - slot)
            else:
                self._tickets[dev][3].append(slot)

    @property
    def lib(self):
        if self._l is None:
            self._l = _lib.load(self._lib_path)
        return self._l

    # ---- host-only helpers (no GPU needed) ----
    def _x3(self):
        """Flag bit 7 of the GEMM entry points: this fp32 launch may take the three-term split."""
        return 128 if (self.fp32_split and self.precision == "fp32") else 0

    def _all16_flags(self):
        """Flags of a launch whose two operands are both 16-bit in HBM, in the current storage mode."""
        return 1 | 2 | 16 | (32 if self.precision == "fp16s" else 0)

    def _query_flags(self, all16=False, planes=False):
        """Flag word (as mmdyn_igemm_nt_mx) under which the host queries see a launch of the current precision mode: plane
        operands, fp32 (with bit 7 where the split is allowed), both operands 16-bit in HBM, or the 16-bit matrix cores on
        anything else."""
        if planes:
            return 384
        if self.precision == "fp32":
            return self._x3()
        if all16 and self.precision in ("bf16s", "fp16s"):
            return self._all16_flags()
        return 1

    def igemm_stat_tiles(self, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, all16=False, planes=False):
        """T of the per-tile BatchNorm partial sums the implicit GEMM of the current precision mode writes.  ``all16``: both
        operands of the launch are 16-bit in HBM (the convolution-level launches of the "bf16s" / "fp16s" modes); ``planes``: the
        fp32x3 launch takes its operands already split (ops.Planes)."""
        return self.lib.mmdyn_igemm_stat_tiles_mx(mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, self._query_flags(all16, planes))

    def colstats_tiles(self, rows_per_group):
        return self.lib.mmdyn_colstats_tiles(rows_per_group)

    def wgrad_chunks(self, mode, rows, Cd, Cg, planes=(False, False)):
        """``planes``: which of (D, Gt) arrive split (ops.Planes): the cut follows the kernel that serves the launch."""
        # (16-bit storage modes: the all-16-bit weight-gradient kernels keep their own tile rule)
        pre = (256 if planes[0] else 0) | (512 if planes[1] else 0)
        r = self.lib.mmdyn_wgrad_chunks_mx(mode, rows, Cd, Cg, 7 if self.precision in ("bf16s", "fp16s") else (self._x3() | (pre if self._x3() else 0)))
        if r < 0:
            check(r, "mmdyn_wgrad_chunks_mx")
        return r

    # ---- GEMMs ----
    def _slabs(self, like, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, all16=False, planes=False):
        """Workspace for the pieces of the persistent ring kernel's split tiles (fp32 launches not split over K), or None."""
        n = self.lib.mmdyn_igemm_slab_floats_mx(mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, self._query_flags(all16, planes))
        return torch.empty(n, device=like.device, dtype=torch.float32) if n > 0 else None

    def _mx(self, *fmts):
        """Base flags of the mixed-storage GEMM entry points: bit 0 (16-bit matrix cores), bit 5 when the 16-bit tensors of
        the call are IEEE half.  The storage format has to be the precision mode's: bf16 tensors with "bf16" / "bf16s",
        half tensors with "fp16s"."""
        half = _half(*fmts)
        ok = ("fp16s",) if half else ("bf16", "bf16s")
        if self.precision not in ok:
            raise ValueError(f"mmdyn_hip: {'fp16' if half else 'bf16'} tensors need precision {' / '.join(ok)} "
                             f"(current: {self.precision})")
        return 1 | (32 if half else 0)

    def _check_stat_tiles(self, stats, all16, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, planes=False):
        """The partial-sum buffer must have the tile count the kernel that serves THIS launch writes (it depends on the
        storage types of the operands: igemm_stat_tiles(..., all16)) -- a mismatch would be an out-of-bounds write."""
        if stats is None:
            return
        T = self.igemm_stat_tiles(mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, all16=all16, planes=planes)
        if stats.dim() != 4 or tuple(stats.shape) != (G, T, 2, N):
            raise ValueError(f"mmdyn_hip: stats must be [G={G}][T={T}][2][N={N}] for this launch (igemm_stat_tiles with "
                             f"all16={all16}), got {tuple(stats.shape)}")

    def _planes_pair(self, A, Bp, Cin):
        """Both operands of a GEMM arrive split (or neither): their pointers, after the checks the kernel cannot make."""
        if not (isinstance(A, Planes) and isinstance(Bp, Planes)):
            raise TypeError("mmdyn_hip: a GEMM takes both operands as Planes or neither")
        if not self._x3():
            raise ValueError("mmdyn_hip: plane operands belong to the fp32x3 arithmetic (engine precision 'fp32x3')")
        if A.C != Cin or Bp.C != Cin:
            raise ValueError(f"mmdyn_hip: plane rows of {A.C} / {Bp.C} channels for a GEMM over Cin = {Cin}")
        for t in (A.t, Bp.t):
            if not t.is_cuda or not t.is_contiguous():
                raise RuntimeError("mmdyn_hip: plane tensors must be contiguous GPU tensors")
        return A.t.data_ptr(), Bp.t.data_ptr()

    def split_planes(self, x, planes):
        """planes <- the exact three-term bf16 split of the fp32 matrix x ([rows][C] contiguous)."""
        if x.numel() != planes.rows * planes.C:
            raise ValueError("mmdyn_hip: split_planes: shapes differ")
        check(self.lib.mmdyn_split_planes(_ptr(x), planes.t.data_ptr(), planes.rows, planes.C, _stream()), "mmdyn_split_planes")

    def igemm_planes_served(self, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N):
        """True when the fp32x3 launch of this shape can take its operands already split (host query, no GPU needed)."""
        return bool(self._x3()) and self.lib.mmdyn_igemm_planes_served(mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N) == 1

    def igemm_nt(self, A, Bp, bias, C, C_act, stats, ws, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, ldc, stride,
                 offset, act, splitk):
        if isinstance(A, Planes) or isinstance(Bp, Planes):
            pa, pb = self._planes_pair(A, Bp, Cin)
            self._check_stat_tiles(stats, False, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, planes=True)
            if ws is None and splitk == 1:
                ws = self._slabs(C, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, planes=True)
            flags, pca = 384, None
            if isinstance(C_act, Planes):            # the activated output as a plane tensor (flag bit 10: DENSE launches)
                if N % C_act.C or C_act.rows * C_act.C != G * Bg * Ho * Wo * N or ldc != N:
                    raise ValueError("mmdyn_hip: igemm_nt: plane output of the wrong shape")
                flags, pca = 384 | 1024 | ((C_act.C // 8) << 16), C_act.t.data_ptr()
            elif C_act is not None:
                pca = _ptr(C_act)
            check(self.lib.mmdyn_igemm_nt_mx(pa, pb, _ptr(bias), _ptr(C), pca, _ptr(stats), _ptr(ws), None, None, None, None,
                                             None, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, ldc, stride, offset, act, splitk, flags,
                                             self._flags(C) if ws is not None and splitk == 1 else None, _stream()), "mmdyn_igemm_nt_mx")
            return
        (pa, a16), (pc, c16), (pca, ca16), (pb, b16) = _aptr(A), _aptr(C), _aptr(C_act), _aptr(Bp)
        self._check_stat_tiles(stats, bool(a16 and b16), mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N)
        if a16 or c16 or ca16 or b16:      # bf16 activation storage / bf16 packed weights: the mixed-storage entry point
            mixed_out = C_act is not None and ca16 and not c16       # fp32 pre-activation + bf16 activated output
            if ((c16 or mixed_out) and splitk != 1) or (C_act is not None and c16 and not ca16):
                raise ValueError("mmdyn_hip: no split-K into a 16-bit output, and a 16-bit C only with a 16-bit C_act")
            if ws is None and splitk == 1:
                ws = self._slabs(A, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, all16=bool(a16 and b16))
            check(self.lib.mmdyn_igemm_nt_mx(pa, pb, _ptr(bias), pc, pca, _ptr(stats), _ptr(ws), None, None, None,
                                             None, None, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, ldc, stride, offset, act,
                                             splitk, self._mx(a16, c16, ca16, b16) | (2 if a16 else 0) | (4 if c16 else 0) |
                                             (16 if b16 else 0) | (64 if mixed_out else 0),
                                             self._flags(C) if ws is not None and splitk == 1 else None, _stream()), "mmdyn_igemm_nt_mx")
            return
        fn = {"fp32": self.lib.mmdyn_igemm_nt, "fp16": self.lib.mmdyn_igemm_nt_f16,
              "fp16s": self.lib.mmdyn_igemm_nt_f16}.get(self.precision, self.lib.mmdyn_igemm_nt_bf16)
        if ws is None and splitk == 1:
            ws = self._slabs(A, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N)
        if self._x3():
            check(self.lib.mmdyn_igemm_nt_mx(pa, pb, _ptr(bias), pc, pca, _ptr(stats), _ptr(ws), None, None, None, None, None,
                                             mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, ldc, stride, offset, act, splitk, 128,
                                             self._flags(C) if ws is not None and splitk == 1 else None, _stream()), "mmdyn_igemm_nt_mx")
            return
        check(fn(pa, _ptr(Bp), _ptr(bias), pc, pca, _ptr(stats), _ptr(ws),
                 mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, ldc, stride, offset, act, splitk, _stream()), "mmdyn_igemm_nt")

    def igemm_nt_dgrad_bn(self, A, Bp, C, stats, y, mean, rstd, gamma, beta, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N,
                          stride, offset):
        if isinstance(A, Planes) or isinstance(Bp, Planes):
            pa, pb = self._planes_pair(A, Bp, Cin)
            self._check_stat_tiles(stats, False, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, planes=True)
            ws = self._slabs(C, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, planes=True)
            check(self.lib.mmdyn_igemm_nt_dgrad_bn(pa, pb, _ptr(C), _ptr(stats), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                                   _ptr(beta), mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride, offset, 4, _ptr(ws),
                                                   self._flags(C) if ws is not None else None, _stream()), "mmdyn_igemm_nt_dgrad_bn")
            return
        (pa, a16), (pc, c16), (py, y16), (pb, b16) = _aptr(A), _aptr(C), _aptr(y), _aptr(Bp)
        self._check_stat_tiles(stats, bool(a16 and b16), mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N)
        if a16 or c16 or y16 or b16:
            ws = self._slabs(A, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, all16=bool(a16 and b16))
            check(self.lib.mmdyn_igemm_nt_mx(pa, pb, None, pc, None, _ptr(stats), _ptr(ws), py, _ptr(mean), _ptr(rstd),
                                             _ptr(gamma), _ptr(beta), mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, N, stride,
                                             offset, ACT_NONE, 1, self._mx(a16, c16, y16, b16) | (2 if a16 else 0) | (4 if c16 else 0) |
                                             (8 if y16 else 0) | (16 if b16 else 0), self._flags(C) if ws is not None else None,
                                             _stream()), "mmdyn_igemm_nt_mx")
            return
        ws = self._slabs(A, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N)
        check(self.lib.mmdyn_igemm_nt_dgrad_bn(pa, _ptr(Bp), pc, _ptr(stats), py, _ptr(mean), _ptr(rstd),
                                               _ptr(gamma), _ptr(beta), mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride,
                                               offset, 3 if self._x3() else {"fp32": 0, "fp16": 2, "fp16s": 2}.get(self.precision, 1), _ptr(ws),
                                               self._flags(C) if ws is not None else None, _stream()),
              "mmdyn_igemm_nt_dgrad_bn")

    def igemm_nt_dgrad_act(self, A, Bp, C, u, act, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride, offset):
        """C = (A x Bp) * act'(u): input-gradient GEMM with the activation backward in its epilogue."""
        if isinstance(A, Planes) or isinstance(Bp, Planes):
            pa, pb = self._planes_pair(A, Bp, Cin)
            ws = self._slabs(C, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, planes=True)
            check(self.lib.mmdyn_igemm_nt_dgrad_act(pa, pb, _ptr(C), _ptr(u), int(act), mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride,
                                                    offset, 384, _ptr(ws), self._flags(C) if ws is not None else None, _stream()),
                  "mmdyn_igemm_nt_dgrad_act")
            return
        (pa, a16), (pc, c16), (pu, u16), (pb, b16) = _aptr(A), _aptr(C), _aptr(u), _aptr(Bp)
        flags = {"fp32": self._x3(), "fp16": 32, "fp16s": 32}.get(self.precision, 1)
        if a16 or c16 or u16 or b16:
            flags = self._mx(a16, c16, u16, b16)
        flags |= (2 if a16 else 0) | (4 if c16 else 0) | (8 if u16 else 0) | (16 if b16 else 0)
        ws = self._slabs(A, mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, all16=bool(a16 and b16)) if (flags in (0, 128) or (a16 and b16)) else None
        check(self.lib.mmdyn_igemm_nt_dgrad_act(pa, pb, pc, pu, int(act), mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride, offset,
                                                flags, _ptr(ws), self._flags(C) if ws is not None else None, _stream()),
              "mmdyn_igemm_nt_dgrad_act")

    def igemm_nt_grouped(self, A, Bp, bias, C, C_act, u, G, rows, K, N, act):
        """G dense GEMMs of one shape in one launch: A [G*rows][K], Bp [G][N][K], bias [G][N] | None, C [G*rows][N];
        u (same shape as C): C = (A . Bp^T) * act'(u)."""
        (pa, a16), (pc, c16), (pca, ca16), (pb, b16), (pu, u16) = _aptr(A), _aptr(C), _aptr(C_act), _aptr(Bp), _aptr(u)
        flags = {"fp32": self._x3(), "fp16": 33, "fp16s": 33}.get(self.precision, 1)
        if a16 or c16 or ca16 or b16 or u16:
            flags = self._mx(a16, c16, ca16, b16, u16)
        flags |= (2 if a16 else 0) | (4 if c16 else 0) | (8 if u16 else 0) | (16 if b16 else 0)
        check(self.lib.mmdyn_igemm_nt_grouped(pa, pb, _ptr(bias), pc, pca, pu, G, rows, K, N, int(act), flags, _stream()),
              "mmdyn_igemm_nt_grouped")

    def wgrad_tn_grouped(self, D, Gt, partial, G, rows, Cd, Cg, chunks):
        """partial [chunks][G][Cd][Cg] of G weight-gradient problems whose rows follow one another in D / Gt."""
        (pd, d16), (pg, g16) = _aptr(D), _aptr(Gt)
        flags = {"fp32": self._x3(), "fp16": 33, "fp16s": 33}.get(self.precision, 1)
        if d16 or g16:
            flags = self._mx(d16, g16)
        flags |= (2 if d16 else 0) | (4 if g16 else 0)
        check(self.lib.mmdyn_wgrad_tn_grouped(pd, pg, _ptr(partial), G, rows, Cd, Cg, chunks, flags, _stream()),
              "mmdyn_wgrad_tn_grouped")

    def splitk_reduce(self, ws, bias, C, C_act, splitk, rows, N, act):
        check(self.lib.mmdyn_splitk_reduce(_ptr(ws), _ptr(bias), _ptr(C), _ptr(C_act), splitk, rows, N, act,
                                           _stream()), "mmdyn_splitk_reduce")

    def wgrad_tn(self, D, Gt, partial, mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg, stride, offset, chunks):
        if isinstance(D, Planes) or isinstance(Gt, Planes):
            # fp32x3 with one or both operands arriving split (flag bits 8 / 9): that operand goes to the LDS planes as it is
            if not self._x3() or mode != CONV:
                raise ValueError("mmdyn_hip: plane operands belong to the convolution-level weight gradients of the fp32x3 arithmetic")
            flags, ptrs = 128, []
            for k, (t, C) in enumerate(((D, Cd), (Gt, Cg))):
                if isinstance(t, Planes):
                    if t.C != C or not t.t.is_cuda or not t.t.is_contiguous():
                        raise ValueError("mmdyn_hip: wgrad_tn: plane operand of the wrong shape")
                    flags |= 256 << k
                    ptrs.append(t.t.data_ptr())
                else:
                    ptrs.append(_ptr(t))
            check(self.lib.mmdyn_wgrad_tn_mx(ptrs[0], ptrs[1], _ptr(partial), mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg, stride, offset, chunks,
                                             flags, _stream()), "mmdyn_wgrad_tn_mx")
            return
        (pd, d16), (pg, g16) = _aptr(D), _aptr(Gt)
        if d16 or g16:
            check(self.lib.mmdyn_wgrad_tn_mx(pd, pg, _ptr(partial), mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg, stride, offset, chunks,
                                             self._mx(d16, g16) | (2 if d16 else 0) | (4 if g16 else 0), _stream()),
                  "mmdyn_wgrad_tn_mx")
            return
        if self._x3():
            check(self.lib.mmdyn_wgrad_tn_mx(pd, pg, _ptr(partial), mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg, stride, offset, chunks, 128,
                                             _stream()), "mmdyn_wgrad_tn_mx")
            return
        fn = {"fp32": self.lib.mmdyn_wgrad_tn, "fp16": self.lib.mmdyn_wgrad_tn_f16,
              "fp16s": self.lib.mmdyn_wgrad_tn_f16}.get(self.precision, self.lib.mmdyn_wgrad_tn_bf16)
        check(fn(pd, pg, _ptr(partial), mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg, stride, offset, chunks,
                 _stream()), "mmdyn_wgrad_tn")

    def wgrad_reduce(self, partial, canon, chunks, taps, Cd, Cg, cg_canon, perm, beta):
        check(self.lib.mmdyn_wgrad_reduce(_ptr(partial), _ptr(canon), chunks, taps, Cd, Cg, cg_canon, perm,
                                          float(beta), _stream()), "mmdyn_wgrad_reduce")

    def _wgrad_canon_flags(self):
        """Flag word of a dense weight gradient on fp32 operands in the current precision mode (as wgrad_tn_grouped)."""
        return {"fp32": self._x3(), "fp16": 33, "fp16s": 33}.get(self.precision, 1)

    def wgrad_canon_served(self, rows, Cd, Cg, groups=1, D=None, Gt=None):
        """Whether wgrad_tn_canon writes this dense weight gradient (the bits of wgrad_tn / wgrad_tn_grouped + wgrad_reduce).
        ``D`` / ``Gt``: the operands, if at hand -- plane operands and 16-bit tensors are not served."""
        if self.precision in ("bf16s", "fp16s"):        # (the 16-bit storage modes cut their chunks for the all-16-bit kernels)
            return False
        for t in (D, Gt):
            if isinstance(t, Planes) or (t is not None and t.dtype != torch.float32):
                return False
        return self.lib.mmdyn_wgrad_canon_served(rows, Cd, Cg, groups, self._wgrad_canon_flags()) == 1

    def wgrad_tn_canon(self, D, Gt, canon, G, rows, Cd, Cg, cg_canon, perm, beta, chunks):
        """canon [G*Cd][cg_canon] (+ beta * canon) of G dense weight-gradient problems whose rows follow one another in D / Gt:
        one launch, no slabs; ``chunks`` as wgrad_chunks(DENSE, rows, Cd, Cg)."""
        check(self.lib.mmdyn_wgrad_tn_canon(_ptr(D), _ptr(Gt), _ptr(canon), G, rows, Cd, Cg, cg_canon, perm, float(beta), chunks,
                                            self._wgrad_canon_flags(), _stream()), "mmdyn_wgrad_tn_canon")

    # ---- packing / layout ----
    def pack_conv_weight(self, Wc, P, d0, d1, swap):
        pp, p16 = _aptr(P)                 # a 16-bit destination: the GEMM operand type of the 16-bit precision modes
        if p16:
            check(self.lib.mmdyn_pack_conv_weight_b16(_ptr(Wc), pp, d0, d1, int(swap), _half(p16), _stream()),
                  "mmdyn_pack_conv_weight_b16")
            return
        check(self.lib.mmdyn_pack_conv_weight(_ptr(Wc), pp, d0, d1, int(swap), _stream()), "mmdyn_pack_conv_weight")

    def repack2d(self, src, dst, rows_in, cols_in, rows_out, cols_out, mode):
        if _is16(dst):
            return self.repack2d_ld(src, dst, rows_in, cols_in, rows_out, cols_out, cols_out, mode)
        check(self.lib.mmdyn_repack2d(_ptr(src), _ptr(dst), rows_in, cols_in, rows_out, cols_out, mode, _stream()),
              "mmdyn_repack2d")

    def repack2d_ld(self, src, dst, rows_in, cols_in, rows_out, cols_out, ld_out, mode):
        """dst: any fp32 (or 16-bit) view whose first element is the block's top-left corner (row stride ld_out)."""
        _, d16 = _aptr(dst)                # device / contiguity / dtype check
        if d16:
            check(self.lib.mmdyn_repack2d_ld_b16(_ptr(src), dst.data_ptr(), rows_in, cols_in, rows_out, cols_out, ld_out, mode,
                                                 _half(d16), _stream()), "mmdyn_repack2d_ld_b16")
            return
        check(self.lib.mmdyn_repack2d_ld(_ptr(src), dst.data_ptr(), rows_in, cols_in, rows_out, cols_out, ld_out, mode,
                                         _stream()), "mmdyn_repack2d_ld")

    def concat_condition(self, x, cond, out, K, cd, bad_index=None):
        """out [rows][width] = [x[:, :K] | condition | 0] in one launch (mmdyn_concat_condition).  ``x``: fp32 rows of unit element
        stride (any row stride >= K); ``cond``: fp32 [rows][cd] (real-valued) or int64 [rows] (categorical: the kernel writes the
        one-hot row); ``bad_index``: int32 [1], bit 0 is set when an index lies outside [0, cd) (that row's block is all zero)."""
        rows, width = out.shape
        ldx, index = self._concat_operands("mmdyn_concat_condition", x, cond, rows, rows, K, cd)
        check(self.lib.mmdyn_concat_condition(x.data_ptr(), None if index else _ptr(cond), _ptr(cond, torch.int64) if index else None,
                                              _ptr(out), _ptr(bad_index, torch.int32), rows, K, ldx, cd, width, _stream()),
              "mmdyn_concat_condition")

    @staticmethod
    def _concat_operands(name, x, cond, rows, x_rows, K, cd):
        """The checks of the two joins: (row stride of x, whether the condition is class indices)."""
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != x_rows or x.shape[1] < K or \
                (x.stride(1) != 1 and x.shape[1] > 1) or (x_rows > 1 and x.stride(0) < K):
            raise ValueError(f"{name}: x must be fp32 GPU rows [{'x_rows' if x_rows != rows else 'rows'}][>= K] of unit element stride")
        index = cond.dtype == torch.int64
        if tuple(cond.shape) != ((rows,) if index else (rows, cd)):
            raise ValueError(f"{name}: condition {tuple(cond.shape)} ({cond.dtype}) does not match rows={rows}, cd={cd}")
        return (x.stride(0) if x_rows > 1 else max(x.stride(0), K)), index

    def concat_condition_tiled(self, x, cond, out, K, cd, x_rows, bad_index=None):
        """concat_condition with ``x`` holding ``x_rows`` rows: out row r = [x[r % x_rows][:K] | condition of row r | 0]
        (mmdyn_concat_condition_tiled).  ``cond`` keeps one entry per out row; rows must be a multiple of x_rows."""
        rows, width = out.shape
        x_rows = int(x_rows)
        if x_rows < 1 or rows % x_rows:
            raise ValueError(f"mmdyn_concat_condition_tiled: rows={rows} is not a multiple of x_rows={x_rows}")
        ldx, index = self._concat_operands("mmdyn_concat_condition_tiled", x, cond, rows, x_rows, K, cd)
        check(self.lib.mmdyn_concat_condition_tiled(x.data_ptr(), None if index else _ptr(cond),
                                                    _ptr(cond, torch.int64) if index else None, _ptr(out),
                                                    _ptr(bad_index, torch.int32), rows, x_rows, K, ldx, cd, width, _stream()),
              "mmdyn_concat_condition_tiled")

    def pack_plan(self, plan_dev, n):
        """plan_dev: uint8 device tensor holding n mmdyn_pack_entry structs (see layers.PackPlan)."""
        check(self.lib.mmdyn_pack_plan(_ptr(plan_dev, torch.uint8), n, _stream()), "mmdyn_pack_plan")

    def im2col_nchw3(self, x, col, Bt, H, W):
        check(self.lib.mmdyn_im2col_nchw3(_ptr(x), _ptr(col), Bt, H, W, _stream()), "mmdyn_im2col_nchw3")

    def col2im_k4(self, col, out, Bt, Hi, Wi, Ho, Wo, C, ldcol, stride, pad, tap_major):
        check(self.lib.mmdyn_col2im_k4(_ptr(col), _ptr(out), Bt, Hi, Wi, Ho, Wo, C, ldcol, stride, pad,
                                       int(tap_major), _stream()), "mmdyn_col2im_k4")

    def tconv_out3_fwd(self, a, w, out, Bt, Hi, Wi):
        pa, a16 = _aptr(a)
        if a16:
            check(self.lib.mmdyn_tconv_out3_fwd_b16(pa, _ptr(w), _ptr(out), Bt, Hi, Wi, _half(a16), _stream()),
                  "mmdyn_tconv_out3_fwd_b16")
            return
        check(self.lib.mmdyn_tconv_out3_fwd(pa, _ptr(w), _ptr(out), Bt, Hi, Wi, _stream()), "mmdyn_tconv_out3_fwd")

    def tconv_out3_bn_fwd(self, y, mean, rstd, gamma, beta, w, out, G, Bg, Hi, Wi):
        """The last decoder layer on the PRE-BatchNorm tensor y: BatchNorm2d + Swish applied while the input tile is staged."""
        py, y16 = _aptr(y)
        check(self.lib.mmdyn_tconv_out3_bn_fwd(py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(w), _ptr(out), G, Bg, Hi, Wi,
                                               y16, _stream()), "mmdyn_tconv_out3_bn_fwd")

    def tconv_out3_bn_bce(self, y, mean, rstd, gamma, beta, w, logits, logits_group, target, dlogit, loss_slots, slot_of_group,
                          grad_scale, G, Bg, Hi, Wi, mask=None, mask_channels=1, unmasked_slots=None):
        """tconv_out3_bn_fwd with the BCE-with-logits term (sums into loss_slots[slot_of_group[g]], dlogit) in its epilogue; the
        logits are written for group ``logits_group`` only (-1: all groups; ``logits`` None: none)."""
        py, y16 = _aptr(y)
        if len(slot_of_group) != G or tuple(target.shape) != (Bg, 3, 2 * Hi, 2 * Wi):
            raise ValueError("mmdyn_hip: tconv_out3_bn_bce: one slot per group and a [Bg][3][2Hi][2Wi] target")
        if logits is not None and logits.numel() != (G if logits_group < 0 else 1) * Bg * 3 * 4 * Hi * Wi:
            raise ValueError("mmdyn_hip: tconv_out3_bn_bce: logits buffer of the wrong size")
        if dlogit is not None and dlogit.numel() != G * Bg * 3 * 4 * Hi * Wi:
            raise ValueError("mmdyn_hip: tconv_out3_bn_bce: dlogit buffer of the wrong size")
        if mask is not None and tuple(mask.shape) != (Bg, mask_channels, 2 * Hi, 2 * Wi):
            raise ValueError(f"mmdyn_hip: tconv_out3_bn_bce: mask {tuple(mask.shape)} is not [Bg][{mask_channels}][2Hi][2Wi]")
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        check(self.lib.mmdyn_tconv_out3_bn_bce(py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(w), _ptr(logits),
                                               int(logits_group), _ptr(target), _ptr(mask), int(mask_channels), _ptr(dlogit),
                                               loss_slots.data_ptr(), None if unmasked_slots is None else unmasked_slots.data_ptr(),
                                               ctypes.addressof(slots), float(grad_scale), G, Bg, Hi, Wi, y16, _stream()),
              "mmdyn_tconv_out3_bn_bce")

    def tconv_out3_bn_bce_rows(self, y, mean, rstd, gamma, beta, w, logits, logits_group, target, loss_rows, slot_of_group, G, Bg,
                               Hi, Wi, mask=None, mask_channels=1, unmasked_rows=None):
        """tconv_out3_bn_bce in evaluation with one sum per SAMPLE: loss_rows [n_slots][Bg] fp64, loss_rows[slot_of_group[g]][b] +=
        the BCE-with-logits sum over sample b of group g.  No gradient output."""
        py, y16 = _aptr(y)
        if len(slot_of_group) != G or tuple(target.shape) != (Bg, 3, 2 * Hi, 2 * Wi):
            raise ValueError("mmdyn_hip: tconv_out3_bn_bce_rows: one slot per group and a [Bg][3][2Hi][2Wi] target")
        if logits is not None and logits.numel() != (G if logits_group < 0 else 1) * Bg * 3 * 4 * Hi * Wi:
            raise ValueError("mmdyn_hip: tconv_out3_bn_bce_rows: logits buffer of the wrong size")
        if mask is not None and tuple(mask.shape) != (Bg, mask_channels, 2 * Hi, 2 * Wi):
            raise ValueError(f"mmdyn_hip: tconv_out3_bn_bce_rows: mask {tuple(mask.shape)} is not [Bg][{mask_channels}][2Hi][2Wi]")
        n_slots = self._row_slots(loss_rows, Bg, "tconv_out3_bn_bce_rows")
        if unmasked_rows is not None and self._row_slots(unmasked_rows, Bg, "tconv_out3_bn_bce_rows") != n_slots:
            raise ValueError("mmdyn_hip: tconv_out3_bn_bce_rows: unmasked_rows and loss_rows differ in shape")
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        check(self.lib.mmdyn_tconv_out3_bn_bce_rows(py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(w), _ptr(logits),
                                                    int(logits_group), _ptr(target), _ptr(mask), int(mask_channels),
                                                    _ptr(loss_rows, torch.float64), _ptr(unmasked_rows, torch.float64),
                                                    ctypes.addressof(slots), n_slots, G, Bg, Hi, Wi, y16, _stream()),
              "mmdyn_tconv_out3_bn_bce_rows")

    def wgrad_out3_bn(self, y, mean, rstd, gamma, beta, Gt, partial, G, Bg, Hr, chunks):
        """Weight gradient of the last decoder layer with swish(BatchNorm(y)) recomputed on the operand fetch."""
        py, y16 = _aptr(y)
        check(self.lib.mmdyn_wgrad_out3_bn(py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(Gt), _ptr(partial), G, Bg, Hr,
                                           chunks, y16, _stream()), "mmdyn_wgrad_out3_bn")

    def nchw_to_nhwc(self, src, dst, B, C, HW):
        check(self.lib.mmdyn_nchw_to_nhwc(_ptr(src), _ptr(dst), B, C, HW, _stream()), "mmdyn_nchw_to_nhwc")

    def nhwc_to_nchw(self, src, dst, B, C, HW):
        check(self.lib.mmdyn_nhwc_to_nchw(_ptr(src), _ptr(dst), B, C, HW, _stream()), "mmdyn_nhwc_to_nchw")

    # ---- BatchNorm + Swish ----
    def colstats(self, y, partial, G, rows_per_group, C):
        check(self.lib.mmdyn_colstats(_ptr(y), _ptr(partial), G, rows_per_group, C, _stream()), "mmdyn_colstats")

    def bn_finalize(self, partial, mean, rstd, running_mean, running_var, nbt, scratch, G, T, C, rows_per_group,
                    eps, momentum, repeat):
        check(self.lib.mmdyn_bn_finalize(_ptr(partial), _ptr(mean), _ptr(rstd), _ptr(running_mean),
                                         _ptr(running_var), _ptr(nbt, torch.int64), _ptr(scratch, torch.float64),
                                         G, T, C, rows_per_group, eps, momentum, repeat, self._ticket(partial, G * T), _stream()),
              "mmdyn_bn_finalize")

    def bn_swish_fwd(self, y, mean, rstd, gamma, beta, a, G, rows_per_group, C, planes=None):
        """``planes`` (a Planes): the activated tensor is ALSO written already split (``a`` may then be None: planes only)."""
        if planes is not None:
            if planes.rows != G * rows_per_group or planes.C != C:
                raise ValueError("mmdyn_hip: bn_swish_fwd: plane tensor of the wrong shape")
            check(self.lib.mmdyn_bn_swish_fwd_planes(_ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(a),
                                                     planes.t.data_ptr(), G, rows_per_group, C, _stream()), "mmdyn_bn_swish_fwd_planes")
            return
        (py, y16), (pa, a16) = _aptr(y), _aptr(a)
        if y16 != a16:
            raise TypeError("mmdyn_hip: bn_swish_fwd input and output must share the storage type")
        if y16:
            check(self.lib.mmdyn_bn_swish_fwd_b16(py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), pa, G, rows_per_group, C,
                                                  _half(y16), _stream()), "mmdyn_bn_swish_fwd_b16")
            return
        check(self.lib.mmdyn_bn_swish_fwd(py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), pa, G, rows_per_group, C,
                                          _stream()), "mmdyn_bn_swish_fwd")

    def bn_swish_bwd_reduce(self, da, y, mean, rstd, gamma, beta, partial, G, rows_per_group, C):
        (pd, d16), (py, y16) = _aptr(da), _aptr(y)
        if d16 != y16:
            raise TypeError("mmdyn_hip: bn_swish_bwd_reduce operands must share the storage type")
        if y16:
            check(self.lib.mmdyn_bn_swish_bwd_reduce_b16(pd, py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(partial),
                                                         G, rows_per_group, C, _half(y16), _stream()),
                  "mmdyn_bn_swish_bwd_reduce_b16")
            return
        check(self.lib.mmdyn_bn_swish_bwd_reduce(pd, py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(partial), G,
                                                 rows_per_group, C, _stream()), "mmdyn_bn_swish_bwd_reduce")

    def bn_bwd_finalize(self, partial, sums, dgamma, dbeta, scratch, G, T, C, beta_acc):
        check(self.lib.mmdyn_bn_bwd_finalize(_ptr(partial), _ptr(sums), _ptr(dgamma), _ptr(dbeta),
                                             _ptr(scratch, torch.float64), G, T, C, float(beta_acc), self._ticket(partial, G * T),
                                             _stream()), "mmdyn_bn_bwd_finalize")

    def bn_eval_stats(self, running_mean, running_var, mean, rstd, G, C, eps):
        check(self.lib.mmdyn_bn_eval_stats(_ptr(running_mean), _ptr(running_var), _ptr(mean), _ptr(rstd), G, C, eps,
                                           _stream()), "mmdyn_bn_eval_stats")

    def bn_reduce_partials(self, partial, sums, scratch, G, T, C):
        F64 = torch.float64
        check(self.lib.mmdyn_bn_reduce_partials(_ptr(partial), _ptr(sums, F64), _ptr(scratch, F64), G, T, C, _stream()),
              "mmdyn_bn_reduce_partials")

    def bn_finalize_sums(self, sums, mean, rstd, running_mean, running_var, nbt, G, C, n, eps, momentum, repeat):
        check(self.lib.mmdyn_bn_finalize_sums(_ptr(sums, torch.float64), _ptr(mean), _ptr(rstd), _ptr(running_mean),
                                              _ptr(running_var), _ptr(nbt, torch.int64), G, C, n, eps, momentum, repeat,
                                              _stream()), "mmdyn_bn_finalize_sums")

    def bn_bwd_finalize_sums(self, sums, sums_f, dgamma, dbeta, G, C, sums_scale, beta_acc):
        check(self.lib.mmdyn_bn_bwd_finalize_sums(_ptr(sums, torch.float64), _ptr(sums_f), _ptr(dgamma), _ptr(dbeta), G, C,
                                                  float(sums_scale), float(beta_acc), _stream()),
              "mmdyn_bn_bwd_finalize_sums")

    def bn_swish_bwd_apply(self, da, y, mean, rstd, gamma, beta, sums, dy, G, rows_per_group, C, da_is_du=False, planes=None):
        """``planes`` (a Planes): dL/dy is ALSO written already split (``dy`` may then be None: planes only)."""
        if planes is not None:
            if planes.rows != G * rows_per_group or planes.C != C:
                raise ValueError("mmdyn_hip: bn_swish_bwd_apply: plane tensor of the wrong shape")
            check(self.lib.mmdyn_bn_swish_bwd_apply_planes(_ptr(da), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(sums),
                                                           _ptr(dy), planes.t.data_ptr(), G, rows_per_group, C, int(da_is_du), _stream()),
                  "mmdyn_bn_swish_bwd_apply_planes")
            return
        (pd, d16), (py, y16), (po, o16) = _aptr(da), _aptr(y), _aptr(dy)
        if not (d16 == y16 == o16):
            raise TypeError("mmdyn_hip: bn_swish_bwd_apply tensors must share the storage type")
        if y16:
            check(self.lib.mmdyn_bn_swish_bwd_apply_b16(pd, py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(sums), po,
                                                        G, rows_per_group, C, int(da_is_du), _half(y16), _stream()),
                  "mmdyn_bn_swish_bwd_apply_b16")
            return
        check(self.lib.mmdyn_bn_swish_bwd_apply(pd, py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(sums), po, G,
                                                rows_per_group, C, int(da_is_du), _stream()), "mmdyn_bn_swish_bwd_apply")

    # ---- the 3-channel layers' direct kernel with plane-row outputs (fp32x3 on fp32 storage, 64 x 64 images) ----
    @staticmethod
    def _conv3_shapes(name, img, Wp, G, Bg, H, **rows32):
        """The sizes the kernel cannot check: the NCHW image, the packed [32][64] weight, every [rows][32] tensor / plane tensor."""
        rows = G * Bg * (H // 2) ** 2
        if img.numel() != G * Bg * 3 * H * H or Wp.numel() != 32 * 64:
            raise ValueError(f"mmdyn_hip: {name}: image / packed weight of the wrong shape")
        for k, t in rows32.items():
            if isinstance(t, Planes):
                if t.rows != rows or t.C != 32 or not t.t.is_cuda or not t.t.is_contiguous():
                    raise ValueError(f"mmdyn_hip: {name}: {k} must be a contiguous GPU plane tensor of [{rows}][3][32]")
            elif t.numel() != rows * 32:
                raise ValueError(f"mmdyn_hip: {name}: {k} must hold [{rows}][32] elements")

    def conv3_fwd_planes(self, x, Wp, C, act_planes, G, Bg, H, act):
        """Conv2d(3, 32, 4, 2, 1) forward: C = the fp32 pre-activation, ``act_planes`` (a Planes) = act(C) already split."""
        self._conv3_shapes("conv3_fwd_planes", x, Wp, G, Bg, H, C=C, act_planes=act_planes)
        check(self.lib.mmdyn_conv3_fwd_planes(_ptr(x), _ptr(Wp), _ptr(C), act_planes.t.data_ptr(), G, Bg, H, int(act), _stream()),
              "mmdyn_conv3_fwd_planes")

    def conv3_dgrad_bn_stats(self, dlogits, Wp, stats, y, mean, rstd, gamma, beta, G, Bg, H):
        """Statistics pass of the last decoder layer's input gradient: the partial-sum table of igemm_nt_dgrad_bn, no du."""
        self._conv3_shapes("conv3_dgrad_bn_stats", dlogits, Wp, G, Bg, H, y=y)
        self._check_stat_tiles(stats, False, IM2COL3, G, Bg, H, H, 64, H // 2, H // 2, 32)
        if mean.numel() != G * 32 or rstd.numel() != G * 32 or gamma.numel() != 32 or beta.numel() != 32:
            raise ValueError("mmdyn_hip: conv3_dgrad_bn_stats: BatchNorm vectors of the wrong shape")
        check(self.lib.mmdyn_conv3_dgrad_bn_stats(_ptr(dlogits), _ptr(Wp), _ptr(stats), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                                  _ptr(beta), G, Bg, H, _stream()), "mmdyn_conv3_dgrad_bn_stats")

    def conv3_dgrad_bn_apply_planes(self, dlogits, Wp, y, mean, rstd, gamma, beta, sums, dy_planes, G, Bg, H):
        """Apply pass: du recomputed, dL/dy written as ``dy_planes`` (a Planes) from the finalized ``sums`` [G][2][32]."""
        self._conv3_shapes("conv3_dgrad_bn_apply_planes", dlogits, Wp, G, Bg, H, y=y, dy_planes=dy_planes)
        if mean.numel() != G * 32 or rstd.numel() != G * 32 or gamma.numel() != 32 or beta.numel() != 32 or sums.numel() != G * 64:
            raise ValueError("mmdyn_hip: conv3_dgrad_bn_apply_planes: BatchNorm vectors / sums of the wrong shape")
        check(self.lib.mmdyn_conv3_dgrad_bn_apply_planes(_ptr(dlogits), _ptr(Wp), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                                         _ptr(beta), _ptr(sums), dy_planes.t.data_ptr(), G, Bg, H, _stream()),
              "mmdyn_conv3_dgrad_bn_apply_planes")

    def bn_eval_swish_bwd(self, da, y, mean, rstd, gamma, beta, dy, partial, G, rows_per_group, C, da_is_du=False, planes=None):
        """Backward of eval-mode BatchNorm + Swish in one pass: dy = du * gamma * rstd -> ``dy`` (fp32) and / or ``planes`` (a
        Planes); ``partial`` (nullable) [G][colstats_tiles][2][C]: the tile sums bn_bwd_finalize turns into dgamma / dbeta.  With
        ``da_is_du`` and no ``partial``, ``y`` is not read and may be None.  fp32 only."""
        if planes is not None and (planes.rows != G * rows_per_group or planes.C != C):
            raise ValueError("mmdyn_hip: bn_eval_swish_bwd: plane tensor of the wrong shape")
        n = G * rows_per_group * C
        for t in (da, y, dy):
            if t is not None and t.numel() != n:
                raise ValueError("mmdyn_hip: bn_eval_swish_bwd: da / y / dy must hold G * rows_per_group * C elements")
        if partial is not None and partial.numel() != G * self.colstats_tiles(rows_per_group) * 2 * C:
            raise ValueError("mmdyn_hip: bn_eval_swish_bwd: partial must be [G][colstats_tiles(rows_per_group)][2][C]")
        if mean.numel() != G * C or rstd.numel() != G * C or gamma.numel() != C or beta.numel() != C:
            raise ValueError("mmdyn_hip: bn_eval_swish_bwd: mean / rstd are [G][C], gamma / beta [C]")
        check(self.lib.mmdyn_bn_eval_swish_bwd(_ptr(da), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(dy),
                                               None if planes is None else planes.t.data_ptr(), _ptr(partial), G, rows_per_group, C,
                                               int(da_is_du), _stream()), "mmdyn_bn_eval_swish_bwd")

    # ---- element-wise ----
    def act_fwd(self, u, h, act):
        check(self.lib.mmdyn_act_fwd(_ptr(u), _ptr(h), u.numel(), act, _stream()), "mmdyn_act_fwd")

    def act_bwd(self, dh, u, du, act):
        (pd, d16), (pu, u16), (po, o16) = _aptr(dh), _aptr(u), _aptr(du)
        if not (d16 == u16 == o16):
            raise TypeError("mmdyn_hip: act_bwd tensors must share the storage type")
        if u16:
            check(self.lib.mmdyn_act_bwd_b16(pd, pu, po, u.numel(), act, _half(u16), _stream()), "mmdyn_act_bwd_b16")
            return
        check(self.lib.mmdyn_act_bwd(pd, pu, po, u.numel(), act, _stream()), "mmdyn_act_bwd")

    def dropout_expand(self, h, masks, out, P, B, H, p_drop):
        check(self.lib.mmdyn_dropout_expand(_ptr(h), _ptr(masks, torch.uint8), _ptr(out), P, B, H, p_drop,
                                            _stream()), "mmdyn_dropout_expand")

    def dropout_reduce(self, dout, masks, dh, P, B, H, p_drop, u=None, act=ACT_NONE, planes=None):
        """u (optional, [B][H] fp32): dh = (sum over the passes) * act'(u) -- the activation backward in the same launch.
        planes (optional ops.Planes [B][H]): dh is written there as well, already split."""
        if planes is not None and (planes.rows != B or planes.C != H):
            raise ValueError("mmdyn_hip: dropout_reduce: plane output of the wrong shape")
        check(self.lib.mmdyn_dropout_reduce(_ptr(dout), _ptr(masks, torch.uint8), _ptr(dh), P, B, H, p_drop,
                                            _ptr(u), int(act), None if planes is None else planes.t.data_ptr(), _stream()),
              "mmdyn_dropout_reduce")

    def random_masks(self, masks, p_drop, seed, offset, offset_dev=None):
        check(self.lib.mmdyn_random_masks(_ptr(masks, torch.uint8), masks.numel(), p_drop, seed, offset,
                                          _ptr(offset_dev, torch.int64), _stream()), "mmdyn_random_masks")

    def random_normal(self, out, seed, offset, offset_dev=None):
        check(self.lib.mmdyn_random_normal(_ptr(out), out.numel(), seed, offset, _ptr(offset_dev, torch.int64),
                                           _stream()), "mmdyn_random_normal")

    def counter_add(self, counter, inc):
        check(self.lib.mmdyn_counter_add(_ptr(counter, torch.int64), inc, _stream()), "mmdyn_counter_add")

    def colsum(self, x, out, rows, C, perm, beta):
        scratch = torch.empty(self.lib.mmdyn_colsum_chunks(rows) * C, device=x.device, dtype=torch.float32)
        check(self.lib.mmdyn_colsum(_ptr(x), _ptr(out), _ptr(scratch), rows, C, perm, float(beta), self._ticket(x),
                                    _stream()), "mmdyn_colsum")

    def scale_dev(self, x, s, out):
        check(self.lib.mmdyn_scale_dev(_ptr(x), _ptr(s), _ptr(out), x.numel(), _stream()), "mmdyn_scale_dev")

    def sum_blocks(self, x, out, P, n):
        check(self.lib.mmdyn_sum_blocks(_ptr(x), _ptr(out), P, n, _stream()), "mmdyn_sum_blocks")

    def cast_f32_to_bf16(self, src, dst):
        """dst (bf16, same element count) = RNE(src): the gradient bucket on its way to the all-reduce."""
        check(self.lib.mmdyn_cast_f32_to_bf16(_ptr(src), _ptr(dst, torch.bfloat16), src.numel(), _stream()),
              "mmdyn_cast_f32_to_bf16")

    def copy_many(self, pairs):
        """[(dst, src)]: contiguous GPU tensors of equal byte size, copied by ONE launch per 8 pairs."""
        pairs = [(d, s_) for d, s_ in pairs if d.data_ptr() != s_.data_ptr()]
        for d, s_ in pairs:
            if not (d.is_cuda and s_.is_cuda and d.is_contiguous() and s_.is_contiguous()) or \
                    d.numel() * d.element_size() != s_.numel() * s_.element_size() or d.dtype != s_.dtype:
                raise ValueError("mmdyn_hip: copy_many takes contiguous GPU tensors of equal type and size")
        for i in range(0, len(pairs), 8):
            part = pairs[i:i + 8]
            n = len(part)
            src = (ctypes.c_void_p * n)(*[s_.data_ptr() for _, s_ in part])
            dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in part])
            nb = (ctypes.c_int64 * n)(*[d.numel() * d.element_size() for d, _ in part])
            check(self.lib.mmdyn_copy_many(ctypes.addressof(src), ctypes.addressof(dst), ctypes.addressof(nb), n, _stream()),
                  "mmdyn_copy_many")

    def cast_bf16_to_f32(self, src, dst):
        check(self.lib.mmdyn_cast_bf16_to_f32(_ptr(src, torch.bfloat16), _ptr(dst), src.numel(), _stream()),
              "mmdyn_cast_bf16_to_f32")

    def linear_small_fwd(self, x, W, b, y, rows, K, N, act):
        check(self.lib.mmdyn_linear_small_fwd(_ptr(x), _ptr(W), _ptr(b), _ptr(y), rows, K, N, act, _stream()),
              "mmdyn_linear_small_fwd")

    def linear_small_bwd(self, dy, x, W, dx, dW, db, rows, K, N, beta):
        check(self.lib.mmdyn_linear_small_bwd(_ptr(dy), _ptr(x), _ptr(W), _ptr(dx), _ptr(dW), _ptr(db), rows, K, N,
                                              float(beta), _stream()), "mmdyn_linear_small_bwd")

    # ---- latent / loss ----
    @staticmethod
    def _passes(passes):
        """passes: list of dicts {'mu': [t|None]*n, 'lv': [...], 'dmu': [...], 'dlv': [...], 'ld': [int]*n}, n<=4;
        tensors may be views (row stride ld) into the fused heads output, so raw data_ptr is used."""
        arr = (PassExperts * MAX_PASSES)()
        for i, p in enumerate(passes):
            for m in range(len(p["ld"])):
                for key in ("mu", "lv", "dmu", "dlv"):
                    t = p.get(key, [None] * MAX_EXPERTS)[m]
                    if t is not None:
                        if not t.is_cuda or t.dtype != torch.float32 or t.stride(-1) != 1:
                            raise ValueError("mmdyn_hip: expert tensors must be fp32 GPU tensors with unit inner stride")
                        getattr(arr[i], key)[m] = t.data_ptr()
                arr[i].ld[m] = int(p["ld"][m])
            for k, t in enumerate(p.get("dz", [])):
                if t is not None:
                    arr[i].dz[k] = _ptr(t)
            for k, t in enumerate(p.get("zdst", [])):      # forward: further [B][L] destinations of the pass's z
                if t is not None:
                    arr[i].zdst[k] = _ptr(t)
            for k, t in enumerate(p.get("zpl", [])):       # ... and plane row blocks (raw pointers into an ops.Planes)
                if t is not None:
                    arr[i].zpl[k] = int(t)
        return arr

    def poe_fwd(self, passes, eps_noise, mu, logvar, z, kl_sum, with_prior, P, B, L):
        arr = self._passes(passes)
        check(self.lib.mmdyn_poe_fwd(ctypes.cast(arr, ctypes.c_void_p), _ptr(eps_noise), _ptr(mu), _ptr(logvar),
                                     _ptr(z), _ptr(kl_sum, torch.float64), int(with_prior), P, B, L, _stream()),
              "mmdyn_poe_fwd")

    def poe_bwd(self, passes, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale, with_prior, P, B, L, kl_weight_dev=None):
        """kl_weight_dev: optional 1-element device tensor multiplying kl_scale (the annealed KL weight kept on the GPU)."""
        arr = self._passes(passes)
        check(self.lib.mmdyn_poe_bwd(ctypes.cast(arr, ctypes.c_void_p), _ptr(eps_noise), _ptr(mu), _ptr(logvar),
                                     _ptr(dz), _ptr(g_mu), _ptr(g_lv), float(kl_scale), int(with_prior), P, B, L,
                                     _ptr(kl_weight_dev), _stream()), "mmdyn_poe_bwd")

    def reparam_fwd(self, mu, lv, eps_noise, z, kl_sum, B, L, ld):
        """mu/lv may be column views (row stride ld) of the fused heads output."""
        check(self.lib.mmdyn_reparam_fwd(mu.data_ptr(), lv.data_ptr(), _ptr(eps_noise), _ptr(z),
                                         None if kl_sum is None else kl_sum.data_ptr(), B, L, ld, _stream()),
              "mmdyn_reparam_fwd")

    def reparam_bwd(self, mu, lv, eps_noise, dz, kl_scale, dmu, dlv, B, L, ld):
        check(self.lib.mmdyn_reparam_bwd(mu.data_ptr(), lv.data_ptr(), _ptr(eps_noise), _ptr(dz), float(kl_scale),
                                         dmu.data_ptr(), dlv.data_ptr(), B, L, ld, _stream()), "mmdyn_reparam_bwd")

    def bce_logits(self, logits, target, mask, dlogit, loss_sum, n, chw, hw, grad_scale, mask_channels=1):
        if mask is not None and mask.numel() * chw != n * mask_channels * hw:
            raise ValueError(f"mmdyn_bce_logits: mask of {mask.numel()} elements does not match [B={n // chw}]"
                             f"[{mask_channels}][hw={hw}]")
        check(self.lib.mmdyn_bce_logits(_ptr(logits), _ptr(target), _ptr(mask), _ptr(dlogit),
                                        loss_sum.data_ptr(), n, chw, hw, int(mask_channels), float(grad_scale), _stream()),
              "mmdyn_bce_logits")

    def bce_logits_groups(self, logits, target, dlogit, loss_slots, slot_of_group, n, grad_scale, mask=None, chw=0, hw=0,
                          mask_channels=1, unmasked_slots=None):
        """logits / dlogit: [G*n]; target: [n]; loss_slots: fp64 vector; slot_of_group[g] < 0 = discarded pass.
        mask ([B][mask_channels][hw], n = B*chw): the --mask-loss form; unmasked_slots then also gets the plain sums."""
        G = len(slot_of_group)
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        if mask is None:
            check(self.lib.mmdyn_bce_logits_groups(_ptr(logits), _ptr(target), _ptr(dlogit), loss_slots.data_ptr(),
                                                   ctypes.addressof(slots), G, n, float(grad_scale), _stream()),
                  "mmdyn_bce_logits_groups")
            return
        if chw <= 0 or hw <= 0 or mask.numel() * chw != n * mask_channels * hw:
            raise ValueError(f"mmdyn_bce_logits_groups_masked: mask of {mask.numel()} elements does not match "
                             f"[B={n // max(chw, 1)}][{mask_channels}][hw={hw}]")
        check(self.lib.mmdyn_bce_logits_groups_masked(_ptr(logits), _ptr(target), _ptr(mask), _ptr(dlogit),
                                                      loss_slots.data_ptr(),
                                                      None if unmasked_slots is None else unmasked_slots.data_ptr(),
                                                      ctypes.addressof(slots), G, n, chw, hw, int(mask_channels),
                                                      float(grad_scale), _stream()), "mmdyn_bce_logits_groups_masked")

    def mse(self, r, t, dr, loss_sum, n, grad_scale):
        check(self.lib.mmdyn_mse(_ptr(r), _ptr(t), _ptr(dr), loss_sum.data_ptr(), n, float(grad_scale), _stream()),
              "mmdyn_mse")

    def mse_groups(self, r, t, dr, loss_slots, slot_of_group, n, grad_scale):
        """r / dr: [G*n]; t: [n]; loss_slots: fp64 vector, pass g adds its sum to loss_slots[slot_of_group[g]].  One launch."""
        G = len(slot_of_group)
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        check(self.lib.mmdyn_mse_groups(_ptr(r), _ptr(t), _ptr(dr), loss_slots.data_ptr(), ctypes.addressof(slots), G, n,
                                        float(grad_scale), _stream()), "mmdyn_mse_groups")

    def elbo_assemble(self, bce, mse, kl, loss, partials, P, B, kl_weight, pose_multiplier, kl_weight_dev=None):
        check(self.lib.mmdyn_elbo_assemble(_ptr(bce, torch.float64), _ptr(mse, torch.float64),
                                           _ptr(kl, torch.float64), _ptr(loss), _ptr(partials), P, B,
                                           float(kl_weight), float(pose_multiplier), _ptr(kl_weight_dev), _stream()),
              "mmdyn_elbo_assemble")

    # ---- per-sample ELBO (evaluation only) ----
    @staticmethod
    def _row_slots(rows, Bg, name):
        """Number of slots of a [n_slots][Bg] fp64 row table."""
        if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] != Bg:
            raise ValueError(f"mmdyn_hip: {name}: the row table must be fp64 [n_slots][Bg={Bg}], got {rows.dtype} {tuple(rows.shape)}")
        return rows.shape[0]

    def bce_logits_rows_groups(self, logits, target, rows_out, slot_of_group, Bg, chw, mask=None, hw=0, mask_channels=1,
                               unmasked_rows=None):
        """logits: [G*Bg*chw]; target: [Bg*chw]; rows_out: fp64 [n_slots][Bg], rows_out[slot_of_group[g]][b] += the BCE-with-logits
        sum over sample b of pass g (slot < 0 = discarded pass).  mask ([Bg][mask_channels][hw]): the --mask-loss form;
        unmasked_rows then also gets the plain sums."""
        G = len(slot_of_group)
        n_slots = self._row_slots(rows_out, Bg, "bce_logits_rows_groups")
        if logits.numel() != G * Bg * chw or target.numel() != Bg * chw:
            raise ValueError(f"mmdyn_bce_logits_rows_groups: logits of {logits.numel()} / target of {target.numel()} elements do "
                             f"not match [G={G}][Bg={Bg}][chw={chw}]")
        if mask is not None and (hw <= 0 or mask.numel() != Bg * mask_channels * hw):
            raise ValueError(f"mmdyn_bce_logits_rows_groups: mask of {mask.numel()} elements does not match "
                             f"[Bg={Bg}][{mask_channels}][hw={hw}]")
        if unmasked_rows is not None and self._row_slots(unmasked_rows, Bg, "bce_logits_rows_groups") != n_slots:
            raise ValueError("mmdyn_bce_logits_rows_groups: unmasked_rows and rows_out differ in shape")
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        check(self.lib.mmdyn_bce_logits_rows_groups(_ptr(logits), _ptr(target), _ptr(mask), int(mask_channels),
                                                    _ptr(rows_out, torch.float64), _ptr(unmasked_rows, torch.float64),
                                                    ctypes.addressof(slots), n_slots, G, Bg, chw, hw, _stream()),
              "mmdyn_bce_logits_rows_groups")

    def mse_rows_groups(self, r, t, rows_out, slot_of_group, Bg, n):
        """r: [G*Bg*n]; t: [Bg*n]; rows_out: fp64 [n_slots][Bg], rows_out[slot_of_group[g]][b] += sum_n (r - t)^2."""
        G = len(slot_of_group)
        n_slots = self._row_slots(rows_out, Bg, "mse_rows_groups")
        if r.numel() != G * Bg * n or t.numel() != Bg * n:
            raise ValueError(f"mmdyn_mse_rows_groups: r of {r.numel()} / t of {t.numel()} elements do not match [G={G}][Bg={Bg}][n={n}]")
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        check(self.lib.mmdyn_mse_rows_groups(_ptr(r), _ptr(t), _ptr(rows_out, torch.float64), ctypes.addressof(slots), n_slots, G,
                                             Bg, n, _stream()), "mmdyn_mse_rows_groups")

    def kl_rows(self, mu, logvar, kl_rows, P, B, L):
        """mu / logvar: [P][B][L] (contiguous); kl_rows: fp64 [P][B] = -0.5 * sum_L (1 + lv - mu^2 - exp(lv))."""
        if mu.numel() != P * B * L or logvar.numel() != P * B * L or kl_rows.numel() != P * B:
            raise ValueError(f"mmdyn_kl_rows: tensors do not match [P={P}][B={B}][L={L}]")
        check(self.lib.mmdyn_kl_rows(_ptr(mu), _ptr(logvar), _ptr(kl_rows, torch.float64), P, B, L, _stream()), "mmdyn_kl_rows")

    def elbo_assemble_rows(self, bce_rows, mse_rows, kl_rows, kl_sum, out, partials, P, B, kl_weight, pose_multiplier,
                           kl_weight_dev=None, kl_mode=0):
        """out [B] / partials [P][B] fp32 from the fp64 [P][B] row tables; kl_mode 0: the reference's row (kl_weight * kl_sum[p],
        the batch total, in every row), 1: kl_weight * kl_rows[p][b].  No division by B."""
        for t, n, what in ((bce_rows, P * B, "bce_rows"), (mse_rows, P * B, "mse_rows"), (kl_rows, P * B, "kl_rows"),
                           (kl_sum, P, "kl_sum"), (partials, P * B, "partials"), (out, B, "out")):
            if t is not None and t.numel() < n:
                raise ValueError(f"mmdyn_elbo_assemble_rows: {what} holds {t.numel()} elements, needs {n}")
        check(self.lib.mmdyn_elbo_assemble_rows(_ptr(bce_rows, torch.float64), _ptr(mse_rows, torch.float64),
                                                _ptr(kl_rows, torch.float64), _ptr(kl_sum, torch.float64), _ptr(out),
                                                _ptr(partials), P, B, float(kl_weight), float(pose_multiplier),
                                                _ptr(kl_weight_dev), int(kl_mode), _stream()), "mmdyn_elbo_assemble_rows")

    # ---- mixed-modality batches: per-row availability ----
    @staticmethod
    def _avail(table, B, name, like=None):
        """Pointer of an availability table: uint8 [B][MAX_EXPERTS], contiguous, on the device of ``like``."""
        if table is None:
            return None
        if table.dtype != torch.uint8 or tuple(table.shape) != (B, MAX_EXPERTS) or not table.is_contiguous():
            raise ValueError(f"mmdyn_hip: {name}: the availability table must be a contiguous uint8 [B={B}][{MAX_EXPERTS}] tensor, "
                             f"got {table.dtype} {tuple(table.shape)}")
        if like is not None and table.device != like.device:
            raise ValueError(f"mmdyn_hip: {name}: the availability table lives on {table.device}, the tensors on {like.device}")
        return _ptr(table, torch.uint8)

    def _avail_tables(self, avail, P, B, name, like):
        """avail: None, or a list of P tables / None -> (the host array of P device pointers, or None)."""
        if avail is None:
            return None
        if len(avail) != P:
            raise ValueError(f"mmdyn_hip: {name}: {len(avail)} availability tables for {P} passes")
        return (ctypes.c_void_p * MAX_PASSES)(*[self._avail(t, B, name, like) for t in avail])

    def poe_fwd_avail(self, passes, avail, eps_noise, mu, logvar, z, kl_sum, with_prior, P, B, L):
        """poe_fwd with one availability table per pass (``avail``: list of P uint8 [B][4] tensors / None, or None): expert m takes
        part in row b iff the pass holds it and avail[p][b][m] != 0.  A table needs with_prior."""
        arr = self._passes(passes)
        tabs = self._avail_tables(avail, P, B, "poe_fwd_avail", mu)
        check(self.lib.mmdyn_poe_fwd_avail(ctypes.cast(arr, ctypes.c_void_p), None if tabs is None else ctypes.addressof(tabs),
                                           _ptr(eps_noise), _ptr(mu), _ptr(logvar), _ptr(z), _ptr(kl_sum, torch.float64),
                                           int(with_prior), P, B, L, _stream()), "mmdyn_poe_fwd_avail")

    def poe_bwd_avail(self, passes, avail, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale, with_prior, P, B, L, kl_weight_dev=None):
        """poe_bwd with the tables of poe_fwd_avail; the dmu / dlv row of an absent (row, expert) is written as zeros."""
        arr = self._passes(passes)
        tabs = self._avail_tables(avail, P, B, "poe_bwd_avail", mu)
        check(self.lib.mmdyn_poe_bwd_avail(ctypes.cast(arr, ctypes.c_void_p), None if tabs is None else ctypes.addressof(tabs),
                                           _ptr(eps_noise), _ptr(mu), _ptr(logvar), _ptr(dz), _ptr(g_mu), _ptr(g_lv), float(kl_scale),
                                           int(with_prior), P, B, L, _ptr(kl_weight_dev), _stream()), "mmdyn_poe_bwd_avail")

    def complete_select(self, x, recon, avail, modality, out, logits):
        """out[b] = present(b) ? x[b] : (logits ? sigmoid(recon[b]) : recon[b]); x (may be None: no row present), recon, out: fp32
        [B, ...] of one shape; avail: uint8 [B][4] or None (every row present); modality: the table column."""
        B = recon.shape[0]
        row_len = recon.numel() // max(B, 1)
        if out.shape != recon.shape or (x is not None and x.shape != recon.shape):
            raise ValueError(f"mmdyn_complete_select: x {None if x is None else tuple(x.shape)} / recon {tuple(recon.shape)} / out "
                             f"{tuple(out.shape)} differ in shape")
        if not 0 <= int(modality) < MAX_EXPERTS:
            raise ValueError(f"mmdyn_complete_select: modality {modality} is not a column of the availability table")
        check(self.lib.mmdyn_complete_select(_ptr(x), _ptr(recon), self._avail(avail, B, "complete_select", recon), int(modality),
                                             _ptr(out), B, row_len, int(bool(logits)), _stream()), "mmdyn_complete_select")

    def elbo_assemble_rows_avail(self, bce_rows, mse_rows, kl_rows, kl_sum, out, partials, avail, bce_modality, mse_modality, P, B,
                                 kl_weight, pose_multiplier, kl_weight_dev=None, kl_mode=0):
        """elbo_assemble_rows with the TARGET-availability table ``avail`` (uint8 [B][4]): slot p of bce_rows / mse_rows belongs to
        the target modality bce_modality[p] / mse_modality[p] (negative: always counts); an entry whose target is absent in its row
        is left out of the sums and overwritten with 0."""
        for t, n, what in ((bce_rows, P * B, "bce_rows"), (mse_rows, P * B, "mse_rows"), (kl_rows, P * B, "kl_rows"),
                           (kl_sum, P, "kl_sum"), (partials, P * B, "partials"), (out, B, "out")):
            if t is not None and t.numel() < n:
                raise ValueError(f"mmdyn_elbo_assemble_rows_avail: {what} holds {t.numel()} elements, needs {n}")
        if len(bce_modality) != P or len(mse_modality) != P:
            raise ValueError(f"mmdyn_elbo_assemble_rows_avail: the slot -> modality maps must hold P={P} entries")
        bm = (ctypes.c_int * P)(*[int(v) for v in bce_modality])
        mm = (ctypes.c_int * P)(*[int(v) for v in mse_modality])
        check(self.lib.mmdyn_elbo_assemble_rows_avail(_ptr(bce_rows, torch.float64), _ptr(mse_rows, torch.float64),
                                                      _ptr(kl_rows, torch.float64), _ptr(kl_sum, torch.float64), _ptr(out),
                                                      _ptr(partials), self._avail(avail, B, "elbo_assemble_rows_avail", out),
                                                      ctypes.addressof(bm), ctypes.addressof(mm), P, B, float(kl_weight),
                                                      float(pose_multiplier), _ptr(kl_weight_dev), int(kl_mode), _stream()),
              "mmdyn_elbo_assemble_rows_avail")

    # ---- multi-step rollout: the step's decoder outputs -> the next step's inputs ----
    def rollout_feed(self, groups, obs_avail, B):
        """One launch for up to FEED_GROUPS tensors: ``groups`` is a list of dicts {recon, obs | None, out, logits, column};
        out[b] = observed(b) ? obs[b] : (logits ? sigmoid(recon[b]) : recon[b]) with observed(b) = obs is given and (obs_avail is
        None or obs_avail[b][column] != 0).  recon / obs / out: contiguous fp32 [B, ...] of one shape on one device; obs_avail:
        uint8 [B][4] or None.  Each group's result has the bits of :meth:`complete_select` on the same operands."""
        name, B = "rollout_feed", int(B)
        if not isinstance(groups, (list, tuple)) or not 1 <= len(groups) <= FEED_GROUPS:
            raise ValueError(f"mmdyn_hip: {name}: between 1 and {FEED_GROUPS} groups, got "
                             f"{len(groups) if isinstance(groups, (list, tuple)) else type(groups).__name__}")
        if B < 1:
            raise ValueError(f"mmdyn_hip: {name}: B = {B} must be positive")
        arg = FeedGroups()
        like = groups[0]["recon"]
        for g, grp in enumerate(groups):
            recon, obs, out = grp["recon"], grp.get("obs"), grp["out"]
            for t, what in ((recon, "recon"), (obs, "obs"), (out, "out")):
                if t is None and what == "obs":
                    continue
                if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 1 or t.shape[0] != B:
                    raise ValueError(f"mmdyn_hip: {name}: group {g}: {what} must be a contiguous fp32 tensor of B={B} rows, got "
                                     f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
                if t.shape != recon.shape or t.device != like.device:
                    raise ValueError(f"mmdyn_hip: {name}: group {g}: {what} {tuple(t.shape)} on {t.device} does not match recon "
                                     f"{tuple(recon.shape)} on {like.device}")
            if recon.numel() == 0:
                raise ValueError(f"mmdyn_hip: {name}: group {g}: empty rows")
            if not 0 <= int(grp["column"]) < MAX_EXPERTS:
                raise ValueError(f"mmdyn_hip: {name}: group {g}: column {grp['column']} is not a column of the availability table")
        table = self._avail(obs_avail, B, name, like)
        for g, grp in enumerate(groups):
            arg.recon[g], arg.obs[g], arg.out[g] = _ptr(grp["recon"]), _ptr(grp.get("obs")), _ptr(grp["out"])
            arg.row_len[g], arg.logits[g], arg.column[g] = grp["recon"].numel() // B, int(bool(grp["logits"])), int(grp["column"])
        check(self.lib.mmdyn_rollout_feed(ctypes.addressof(arg), len(groups), table, B, _stream()), "mmdyn_rollout_feed")

    # ---- candidate conditions: the cost table, the winner of each row, the winner's rows ----
    @staticmethod
    def _candidate_kind(name, candidates, N, B, T=None):
        """(index, cd, shape of candidates, shape of best_condition) of a planner's candidates: fp32 with cd reals per row or
        int64 indices; T = None: the one-step layout [N * B], otherwise step-major [T][N * B] with the winner's [B][T]."""
        lead, lead_txt = ((), "") if T is None else ((T,), "[T]")
        if not torch.is_tensor(candidates) or candidates.dtype not in (torch.float32, torch.int64):
            raise ValueError(f"mmdyn_{name}: candidates must be fp32 {lead_txt}[N * B][cd] or int64 {lead_txt}[N * B], got "
                             f"{candidates.dtype if torch.is_tensor(candidates) else type(candidates).__name__}")
        if candidates.dtype == torch.int64:
            return True, 1, lead + (N * B,), (B,) + lead
        if candidates.dim() != len(lead) + 2 or candidates.shape[-1] < 1:
            raise ValueError(f"mmdyn_{name}: real-valued candidates must be {'' if T is None else f'[T = {T}]'}[N * B = {N * B}][cd], "
                             f"got {tuple(candidates.shape)}")
        cd = candidates.shape[-1]
        return False, cd, lead + (N * B, cd), (B,) + lead + (cd,)

    @staticmethod
    def _gather_groups(name, groups, best, N, B, T=None):
        """The checked GatherGroups of :meth:`gather_best` (T = None: src [N * B, ...], out [B, ...]) and of
        :meth:`gather_best_steps` (src [T, N * B, ...], out [T, B, ...])."""
        lead = () if T is None else (T,)
        if not isinstance(groups, (list, tuple)) or not 1 <= len(groups) <= FEED_GROUPS:
            raise ValueError(f"mmdyn_hip: {name}: between 1 and {FEED_GROUPS} groups, got "
                             f"{len(groups) if isinstance(groups, (list, tuple)) else type(groups).__name__}")
        if min(N, B, *lead) < 1:
            raise ValueError(f"mmdyn_hip: {name}: " + (f"N = {N} and B = {B}" if T is None else f"N = {N}, B = {B} and T = {T}") +
                             " must be positive")
        if not torch.is_tensor(best) or best.dtype != torch.int32 or tuple(best.shape) != (B,) or not best.is_contiguous():
            raise ValueError(f"mmdyn_hip: {name}: best must be a contiguous int32 [B={B}] tensor")
        arg, d = GatherGroups(), len(lead) + 1
        for g, grp in enumerate(groups):
            src, out = grp["src"], grp["out"]
            for t, rows, what in ((src, N * B, "src"), (out, B, "out")):
                if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < d or \
                        tuple(t.shape[:d]) != lead + (rows,):
                    raise ValueError(f"mmdyn_hip: {name}: group {g}: {what} must be a contiguous fp32 tensor " +
                                     (f"of {rows} rows" if T is None else f"[T={T}][{rows}][...]") +
                                     f", got {(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
            if src.numel() == 0 or tuple(src.shape[d:]) != tuple(out.shape[d:]) or src.device != best.device or out.device != best.device:
                raise ValueError(f"mmdyn_hip: {name}: group {g}: src {tuple(src.shape)} on {src.device} and out {tuple(out.shape)} on "
                                 f"{out.device} must share a non-empty row shape and the device of best")
        for g, grp in enumerate(groups):
            arg.src[g], arg.out[g] = _ptr(grp["src"]), _ptr(grp["out"])
            arg.row_len[g], arg.logits[g] = grp["out"].numel() // (B * (T or 1)), int(bool(grp["logits"]))
        return arg

    def plan_select(self, bce_rows, mse_rows, kl_rows, tavail, candidates, cost, best, best_cost, best_condition, N, B,
                    pose_multiplier, kl_weight=1.0, kl_weight_dev=None):
        """cost [N][B] fp32 = ((bce_rows[0] + bce_rows[1]) + pose_multiplier * mse_rows) + kl_weight * kl_rows, formed in fp64 in that
        order; best [B] int32 = the candidate of the smallest fp64 cost (ties: the lowest index; NaN never wins; all NaN: -1);
        best_cost [B] fp32; best_condition = the winner's condition.  bce_rows: fp64 [2][N][B] or None; mse_rows: fp64 [N][B] or
        None; kl_rows: fp64 [N][B]; tavail: the target-availability table (uint8 [B][4]) or None -- the N table entries of an
        absent (row, term) are overwritten with 0 and left out.  candidates, candidate-major: fp32 [N * B][cd] with best_condition
        fp32 [B][cd], or int64 [N * B] with best_condition int64 [B]."""
        name, N, B = "plan_select", int(N), int(B)
        if N < 1 or B < 1:
            raise ValueError(f"mmdyn_plan_select: N = {N} and B = {B} must be positive")
        index, cd, *shapes = self._candidate_kind(name, candidates, N, B)
        if any(t is None for t in (kl_rows, cost, best, best_cost, best_condition)):
            raise ValueError("mmdyn_plan_select: kl_rows, cost, best, best_cost and best_condition are required")
        f32, f64, ctype = torch.float32, torch.float64, candidates.dtype
        tp = self._avail(tavail, B, name, cost)
        bp, mp, kp, cp, op, sp, wp, qp = self._iw_tables(
            name, (bce_rows, (2, N, B), "bce_rows", f64), (mse_rows, (N, B), "mse_rows", f64), (kl_rows, (N, B), "kl_rows", f64),
            (candidates, shapes[0], "candidates", ctype), (cost, (N, B), "cost", f32), (best, (B,), "best", torch.int32),
            (best_cost, (B,), "best_cost", f32), (best_condition, shapes[1], "best_condition", ctype))
        check(self.lib.mmdyn_plan_select(bp, mp, kp, tp, None if index else cp, cp if index else None, cd, op, sp, wp,
                                         None if index else qp, qp if index else None, N, B, float(pose_multiplier),
                                         float(kl_weight), _ptr(kl_weight_dev), _stream()), "mmdyn_plan_select")

    def gather_best(self, groups, best, N, B):
        """One launch for up to FEED_GROUPS tensors: ``groups`` is a list of dicts {src, out, logits}; out[b] = f(src[best[b] * B +
        b]) with f = sigmoid where ``logits``, the identity otherwise.  src: contiguous fp32 [N * B, ...]; out: contiguous fp32
        [B, ...] of the same row shape, overlapping no src and no other out of the call; best: int32 [B] -- a row whose index is
        -1 (or anywhere outside [0, N)) is filled with NaN and reads nothing.  A taken row has the bits of :meth:`complete_select` (x = None) on it."""
        N, B = int(N), int(B)
        arg = self._gather_groups("gather_best", groups, best, N, B)
        check(self.lib.mmdyn_gather_best(ctypes.addressof(arg), len(groups), _ptr(best, torch.int32), N, B, _stream()),
              "mmdyn_gather_best")

    # ---- candidate condition sequences over T steps: the weighted total, the winner of each row, the winner's trajectory ----
    def plan_select_steps(self, bce_rows, mse_rows, kl_rows, tavail, step_weight, candidates, cost, step_cost, best, best_cost,
                          best_condition, top, top_cost, N, B, T, Tg, pose_multiplier, kl_weight=1.0, kl_weight_dev=None):
        """:meth:`plan_select` over Tg scored steps (Tg = 1: a final goal; Tg = T: every step): step_cost [Tg][N][B] fp32 = the
        cost of :meth:`plan_select` per step; cost [N][B] fp32 = sum_t step_weight[t] * c_t in fp64, t ascending, nothing fused
        (step_weight None: the plain sum); best / best_cost: the smallest fp64 total under the rules there.  bce_rows: fp64
        [2][Tg][N][B] or None; mse_rows: fp64 [Tg][N][B] or None; kl_rows: fp64 [Tg][N][B]; tavail: uint8 [Tg][B][4] or None;
        step_weight: fp32 [Tg] on the device or None.  candidates, step-major and candidate-major: fp32 [T][N * B][cd] with
        best_condition fp32 [B][T][cd], or int64 [T][N * B] with best_condition int64 [B][T].  top / top_cost (both or neither):
        int32 / fp32 [K][B], K <= PLAN_TOP_MAX -- the K smallest totals in ascending order, -1 / NaN past the non-NaN candidates."""
        name, N, B, T, Tg = "plan_select_steps", int(N), int(B), int(T), int(Tg)
        if N < 1 or B < 1 or T < 1 or Tg not in (1, T):
            raise ValueError(f"mmdyn_plan_select_steps: N = {N}, B = {B} and T = {T} must be positive and Tg = {Tg} be 1 or T")
        index, cd, *shapes = self._candidate_kind(name, candidates, N, B, T)
        if any(t is None for t in (kl_rows, cost, step_cost, best, best_cost, best_condition)):
            raise ValueError("mmdyn_plan_select_steps: kl_rows, cost, step_cost, best, best_cost and best_condition are required")
        if (top is None) != (top_cost is None):
            raise ValueError("mmdyn_plan_select_steps: top and top_cost come together")
        K = 0
        if top is not None:
            K = top.shape[0] if torch.is_tensor(top) and top.dim() == 2 else 0
            if not 1 <= K <= PLAN_TOP_MAX:
                raise ValueError(f"mmdyn_plan_select_steps: top must be int32 [K][B = {B}] with K in [1, {PLAN_TOP_MAX}], got "
                                 f"{tuple(top.shape) if torch.is_tensor(top) else type(top).__name__}")
        f32, f64, i32, ctype = torch.float32, torch.float64, torch.int32, candidates.dtype
        tp = None
        if tavail is not None:
            if not torch.is_tensor(tavail) or tavail.dim() != 3 or tuple(tavail.shape[:2]) != (Tg, B) or not tavail.is_contiguous():
                raise ValueError(f"mmdyn_hip: {name}: the availability tables must be a contiguous uint8 [Tg={Tg}][B={B}][{MAX_EXPERTS}] "
                                 f"tensor, got {tuple(tavail.shape) if torch.is_tensor(tavail) else type(tavail).__name__}")
            tp = self._avail(tavail.view(Tg * B, tavail.shape[2]), Tg * B, name, cost)
        bp, mp, kp, wp, cp, op, scp, sp, bcp, qp, tkp, tcp = self._iw_tables(
            name, (bce_rows, (2, Tg, N, B), "bce_rows", f64), (mse_rows, (Tg, N, B), "mse_rows", f64),
            (kl_rows, (Tg, N, B), "kl_rows", f64), (step_weight, (Tg,), "step_weight", f32), (candidates, shapes[0], "candidates", ctype),
            (cost, (N, B), "cost", f32), (step_cost, (Tg, N, B), "step_cost", f32), (best, (B,), "best", i32),
            (best_cost, (B,), "best_cost", f32), (best_condition, shapes[1], "best_condition", ctype), (top, (K, B), "top", i32),
            (top_cost, (K, B), "top_cost", f32))
        check(self.lib.mmdyn_plan_select_steps(bp, mp, kp, tp, wp, None if index else cp, cp if index else None, cd, op, scp, sp, bcp,
                                               None if index else qp, qp if index else None, tkp, tcp, K, N, B, T, Tg,
                                               float(pose_multiplier), float(kl_weight), _ptr(kl_weight_dev), _stream()),
              "mmdyn_plan_select_steps")

    def gather_best_steps(self, groups, best, N, B, T):
        """:meth:`gather_best` on all T steps in one launch: ``groups`` is a list of dicts {src, out, logits}; out[t][b] =
        f(src[t][best[b] * B + b]).  src: contiguous fp32 [T, N * B, ...]; out: contiguous fp32 [T, B, ...] of the same row shape,
        overlapping no src and no other out of the call; best: int32 [B] -- a row whose index lies outside [0, N) is filled with
        NaN in every step and reads nothing.  The bits of T :meth:`gather_best` calls on the step slices."""
        N, B, T = int(N), int(B), int(T)
        arg = self._gather_groups("gather_best_steps", groups, best, N, B, T)
        check(self.lib.mmdyn_gather_best_steps(ctypes.addressof(arg), len(groups), _ptr(best, torch.int32), N, B, T, _stream()),
              "mmdyn_gather_best_steps")

    # ---- iterative refinement (CEM): the candidates of an iteration, the elites and the refitted distribution ----
    @staticmethod
    def _touch(a, b):
        """Whether the storage ranges of two tensors (None: no) intersect."""
        if a is None or b is None:
            return False
        pa, pb = a.data_ptr(), b.data_ptr()
        return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()

    def _disjoint(self, name, ins, outs, own=()):
        """ValueError where an output of op ``name`` touches an input or another output (``ins`` / ``outs``: specs as in
        :meth:`_check_tables`, None tensors skipped).  own: pairs (i, j) -- output i may be exactly input j."""
        for i, (o, _, what, _) in enumerate(outs):
            for j, (t, _, other, _) in enumerate(ins):
                if self._touch(o, t) and not ((i, j) in own and o.data_ptr() == t.data_ptr()):
                    raise ValueError(f"mmdyn_{name}: {what} overlaps {other}" +
                                     (" (an output may only be exactly its own input)" if own else ""))
            for p, _, other, _ in outs[i + 1:]:
                if self._touch(o, p):
                    raise ValueError(f"mmdyn_{name}: {what} overlaps {other}")

    def _refit(self, name, cost, cand, mean_in, std_in, mean_out, std_out, elite, count, K, N, B, T, alpha, std_min,
               temperature=None, extra=()):
        """The checks of :meth:`plan_refit` and :meth:`plan_refit_weighted` (``temperature`` and the ``extra`` output specs: the
        weighted one's): (cd, the pointers in the order of the entry's arguments)."""
        if B < 1 or T < 1 or not 1 <= N <= REFIT_N_MAX or not 1 <= K <= N:
            raise ValueError(f"mmdyn_{name}: B = {B} and T = {T} must be positive, N = {N} lie in [1, {REFIT_N_MAX}] and "
                             f"K = {K} in [1, N]")
        if not 0.0 <= alpha < 1.0 or not std_min >= 0.0:
            raise ValueError(f"mmdyn_{name}: alpha = {alpha} must lie in [0, 1) and std_min = {std_min} be >= 0")
        if temperature is not None and not 0.0 < temperature < float("inf"):
            raise ValueError(f"mmdyn_{name}: temperature = {temperature} must be finite and > 0")
        if any(t is None for t in (cost, cand, mean_in, std_in, mean_out, std_out)):
            raise ValueError(f"mmdyn_{name}: cost, cand, mean_in, std_in, mean_out and std_out are required")
        if not torch.is_tensor(cand) or cand.dim() != 3 or cand.shape[2] < 1:
            raise ValueError(f"mmdyn_{name}: cand must be fp32 [T = {T}][N * B = {N * B}][cd], got "
                             f"{tuple(cand.shape) if torch.is_tensor(cand) else type(cand).__name__}")
        cd = cand.shape[2]
        if N * B * T * cd >= 1 << 31:
            raise ValueError(f"mmdyn_{name}: N * B * T * cd = {N * B * T * cd} elements reach 2^31")
        f32 = torch.float32
        specs = ((cost, (N, B), "cost", f32), (cand, (T, N * B, cd), "cand", f32), (mean_in, (B, T, cd), "mean_in", f32),
                 (std_in, (B, T, cd), "std_in", f32), (mean_out, (B, T, cd), "mean_out", f32), (std_out, (B, T, cd), "std_out", f32),
                 (elite, (N, B), "elite", torch.uint8), (count, (B,), "count", torch.int32)) + tuple(extra)
        self._check_tables(name, *specs)
        self._disjoint(name, specs[:4], specs[4:], own=((0, 2), (1, 3)))
        return cd, [_ptr(t, dtype) for t, _, _, dtype in specs]

    def plan_sample(self, mean, std, eps, keep, lo, hi, cand, N, B, T):
        """cand [T][N * B][cd] fp32 = the candidates of one refinement iteration: row n * B + b of step t is mean[b][t] + std[b][t] *
        eps[n][b][t] (product and sum each rounded to fp32), slot n = 0 the incumbent -- keep[b][t] where it is given and no NaN,
        mean[b][t] otherwise; its eps is not read --, everything clamped to [lo, hi] per dimension where the bounds are given (a NaN
        stays a NaN).  mean / std / keep: fp32 [B][T][cd]; eps: fp32 [N][B][T][cd]; lo / hi: fp32 [cd], both or neither.  cand
        overlaps no input."""
        name, N, B, T = "plan_sample", int(N), int(B), int(T)
        if N < 1 or B < 1 or T < 1:
            raise ValueError(f"mmdyn_plan_sample: N = {N}, B = {B} and T = {T} must be positive")
        if any(t is None for t in (mean, std, eps, cand)):
            raise ValueError("mmdyn_plan_sample: mean, std, eps and cand are required")
        if (lo is None) != (hi is None):
            raise ValueError("mmdyn_plan_sample: lo and hi come together")
        if not torch.is_tensor(mean) or mean.dim() != 3 or mean.shape[2] < 1:
            raise ValueError(f"mmdyn_plan_sample: mean must be fp32 [B = {B}][T = {T}][cd], got "
                             f"{tuple(mean.shape) if torch.is_tensor(mean) else type(mean).__name__}")
        cd = mean.shape[2]
        if N * B * T * cd >= 1 << 31:
            raise ValueError(f"mmdyn_plan_sample: N * B * T * cd = {N * B * T * cd} elements reach 2^31")
        f32 = torch.float32
        specs = ((mean, (B, T, cd), "mean", f32), (std, (B, T, cd), "std", f32), (eps, (N, B, T, cd), "eps", f32),
                 (keep, (B, T, cd), "keep", f32), (lo, (cd,), "lo", f32), (hi, (cd,), "hi", f32), (cand, (T, N * B, cd), "cand", f32))
        self._check_tables(name, *specs)
        self._disjoint(name, specs[:-1], specs[-1:])
        ptrs = [_ptr(t, dtype) for t, _, _, dtype in specs]
        check(self.lib.mmdyn_plan_sample(*ptrs, N, B, T, cd, _stream()), "mmdyn_plan_sample")

    def plan_refit(self, cost, cand, mean_in, std_in, mean_out, std_out, elite, count, K, N, B, T, alpha=0.0, std_min=0.0):
        """The elites of every row and the distribution refitted to them.  cost: fp32 [N][B] (plan_select_steps); cand: fp32
        [T][N * B][cd]; candidate n is an elite of row b iff cost[n][b] is no NaN and fewer than K candidates come in front of it (a
        smaller cost, or an equal one with a lower n).  Over the K' elites in ascending n, in fp64, each operation rounded on its
        own: m = sum c / K', s = sqrt(sum (c - m)^2 / K'); mean_out = fp32(alpha * mean_in + (1 - alpha) * m), std_out =
        fmax(fp32(alpha * std_in + (1 - alpha) * s), std_min); K' = 0: the inputs, bit for bit.  mean_* / std_*: fp32 [B][T][cd],
        an output may be exactly its input and overlaps nothing else; elite: uint8 [N][B] or None; count: int32 [B] or None."""
        K, N, B, T, alpha, std_min = int(K), int(N), int(B), int(T), float(alpha), float(std_min)
        cd, ptrs = self._refit("plan_refit", cost, cand, mean_in, std_in, mean_out, std_out, elite, count, K, N, B, T, alpha, std_min)
        check(self.lib.mmdyn_plan_refit(*ptrs, K, N, B, T, cd, alpha, std_min, _stream()), "mmdyn_plan_refit")

    # ---- MPPI weights and the receding horizon ----
    def plan_refit_weighted(self, cost, cand, mean_in, std_in, mean_out, std_out, elite, count, weight, ess, K, N, B, T,
                            temperature=1.0, alpha=0.0, std_min=0.0):
        """:meth:`plan_refit` with the weight w_n = exp(-(cost_n - c_min) / temperature) on every elite (c_min: the smallest elite
        cost; exactly 1 where cost_n == c_min, 0 for a non-elite; fp64, each operation rounded on its own).  K == N ranks nothing:
        every candidate whose cost is no NaN is an elite.  W = sum w, Q = sum w^2 in ascending n; m = (sum w c) / W, s =
        sqrt((sum w (c - m)^2) / W) over the candidates of non-zero weight, then plan_refit's blend and floor; K' = 0: the inputs,
        bit for bit.  Equal elite costs: the bits of plan_refit.  weight: fp64 [N][B] or None; ess: fp32 [B] = W^2 / Q (0 when
        K' = 0) or None; neither overlaps anything.  Everything else as in plan_refit."""
        K, N, B, T = int(K), int(N), int(B), int(T)
        temperature, alpha, std_min = float(temperature), float(alpha), float(std_min)
        cd, ptrs = self._refit("plan_refit_weighted", cost, cand, mean_in, std_in, mean_out, std_out, elite, count, K, N, B, T, alpha,
                               std_min, temperature, ((weight, (N, B), "weight", torch.float64), (ess, (B,), "ess", torch.float32)))
        check(self.lib.mmdyn_plan_refit_weighted(*ptrs, K, N, B, T, cd, temperature, alpha, std_min, _stream()),
              "mmdyn_plan_refit_weighted")

    def plan_shift(self, prev_mean, prev_std, prev_keep, init_mean, init_std, mean_out, std_out, keep_out, B, T, shift=1, widen=0.0):
        """The warm start of a horizon that has moved ``shift`` steps on.  Every tensor fp32 [B][T][cd]; prev_keep / keep_out: both or
        neither.  For t + shift < T: mean_out[b][t] = prev_mean[b][t + shift], keep_out likewise, std_out[b][t] =
        fmax(prev_std[b][t + shift], widen * init_std[b][t]) (one fp32 product; fmax takes the other side of a NaN); past that, the
        tail: mean_out = keep_out = init_mean[b][t], std_out = init_std[b][t].  No output overlaps an input or another output."""
        name, B, T, shift, widen = "plan_shift", int(B), int(T), int(shift), float(widen)
        if B < 1 or T < 1 or not 0 <= shift <= T:
            raise ValueError(f"mmdyn_plan_shift: B = {B} and T = {T} must be positive and shift = {shift} lie in [0, T]")
        if not 0.0 <= widen < float("inf"):
            raise ValueError(f"mmdyn_plan_shift: widen = {widen} must be finite and >= 0")
        if any(t is None for t in (prev_mean, prev_std, init_mean, init_std, mean_out, std_out)):
            raise ValueError("mmdyn_plan_shift: prev_mean, prev_std, init_mean, init_std, mean_out and std_out are required")
        if (prev_keep is None) != (keep_out is None):
            raise ValueError("mmdyn_plan_shift: prev_keep and keep_out come together")
        if not torch.is_tensor(prev_mean) or prev_mean.dim() != 3 or prev_mean.shape[2] < 1:
            raise ValueError(f"mmdyn_plan_shift: prev_mean must be fp32 [B = {B}][T = {T}][cd], got "
                             f"{tuple(prev_mean.shape) if torch.is_tensor(prev_mean) else type(prev_mean).__name__}")
        cd = prev_mean.shape[2]
        if B * T * cd >= 1 << 31:
            raise ValueError(f"mmdyn_plan_shift: B * T * cd = {B * T * cd} elements reach 2^31")
        f32 = torch.float32
        specs = tuple((t, (B, T, cd), what, f32) for t, what in (
            (prev_mean, "prev_mean"), (prev_std, "prev_std"), (prev_keep, "prev_keep"), (init_mean, "init_mean"), (init_std, "init_std"),
            (mean_out, "mean_out"), (std_out, "std_out"), (keep_out, "keep_out")))
        self._check_tables(name, *specs)
        self._disjoint(name, specs[:5], specs[5:])
        ptrs = [_ptr(t, dtype) for t, _, _, dtype in specs]
        check(self.lib.mmdyn_plan_shift(*ptrs, B, T, cd, shift, widen, _stream()), "mmdyn_plan_shift")

    # ---- ensemble rollout: the N * B decoder rows of a step -> the N * B next states + the ensemble's statistics ----
    def ensemble_feed(self, groups, obs_avail, N, B):
        """One launch for up to FEED_GROUPS tensors: ``groups`` is a list of dicts {recon, obs | None, out, mean, var | None,
        spread | None, logits, column}.  recon / out: contiguous fp32 [N * B, ...], sample-major (row n * B + b); obs / mean / var:
        contiguous fp32 [B, ...] of the same row shape; spread: contiguous fp64 [B], an accumulator the caller zeroes (needs var);
        obs_avail: uint8 [B][4] or None.  With p = sigmoid(recon) where ``logits``, recon otherwise: out[n * B + b] = observed(b) ?
        obs[b] : p (the bits of :meth:`rollout_feed` on the N * B rows with obs and the table repeated), mean / var = the mean and
        population variance of p over n, spread[b] += sum of var[b]."""
        name, N, B = "ensemble_feed", int(N), int(B)
        if not isinstance(groups, (list, tuple)) or not 1 <= len(groups) <= FEED_GROUPS:
            raise ValueError(f"mmdyn_hip: {name}: between 1 and {FEED_GROUPS} groups, got "
                             f"{len(groups) if isinstance(groups, (list, tuple)) else type(groups).__name__}")
        if N < 1 or B < 1:
            raise ValueError(f"mmdyn_hip: {name}: N = {N} and B = {B} must be positive")
        arg = EnsembleGroups()
        like = groups[0]["recon"]
        for g, grp in enumerate(groups):
            recon, spread = grp["recon"], grp.get("spread")
            for t, rows, what in ((recon, N * B, "recon"), (grp["out"], N * B, "out"), (grp.get("obs"), B, "obs"),
                                  (grp["mean"], B, "mean"), (grp.get("var"), B, "var")):
                if t is None and what in ("obs", "var"):
                    continue
                if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 1 or t.shape[0] != rows:
                    raise ValueError(f"mmdyn_hip: {name}: group {g}: {what} must be a contiguous fp32 tensor of {rows} rows, got "
                                     f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
                if tuple(t.shape[1:]) != tuple(recon.shape[1:]) or t.device != like.device:
                    raise ValueError(f"mmdyn_hip: {name}: group {g}: {what} {tuple(t.shape)} on {t.device} does not match the rows "
                                     f"of recon {tuple(recon.shape)} on {like.device}")
            if recon.numel() == 0:
                raise ValueError(f"mmdyn_hip: {name}: group {g}: empty rows")
            if spread is not None:
                if not torch.is_tensor(spread) or spread.dtype != torch.float64 or tuple(spread.shape) != (B,) or \
                        not spread.is_contiguous() or spread.device != like.device:
                    raise ValueError(f"mmdyn_hip: {name}: group {g}: spread must be a contiguous fp64 [B={B}] tensor on {like.device}")
                if grp.get("var") is None:
                    raise ValueError(f"mmdyn_hip: {name}: group {g}: spread is the row sum of var, which was not given")
            if not 0 <= int(grp["column"]) < MAX_EXPERTS:
                raise ValueError(f"mmdyn_hip: {name}: group {g}: column {grp['column']} is not a column of the availability table")
        table = self._avail(obs_avail, B, name, like)
        for g, grp in enumerate(groups):
            arg.recon[g], arg.obs[g], arg.out[g] = _ptr(grp["recon"]), _ptr(grp.get("obs")), _ptr(grp["out"])
            arg.mean[g], arg.var[g], arg.spread[g] = _ptr(grp["mean"]), _ptr(grp.get("var")), _ptr(grp.get("spread"), torch.float64)
            arg.row_len[g], arg.logits[g], arg.column[g] = grp["mean"].numel() // B, int(bool(grp["logits"])), int(grp["column"])
        check(self.lib.mmdyn_ensemble_feed(ctypes.addressof(arg), len(groups), table, N, B, _stream()), "mmdyn_ensemble_feed")

    def ensemble_quantiles(self, groups, lo, frac, N, B):
        """One launch for up to FEED_GROUPS tensors: ``groups`` is a list of dicts {src, out, logits}.  src: contiguous fp32
        [N * B, ...], sample-major (the ``recon`` of :meth:`ensemble_feed`); out: contiguous fp32 [Q, B, ...] of the same row shape,
        overlapping no src and no other out of the call.  ``lo`` (ints in [0, N)) and ``frac`` (floats in [0, 1)), Q = len(lo) =
        len(frac) in [1, QUANTILES_MAX]: with p = sigmoid(src) where ``logits``, src otherwise, and s the N values of an element in
        ascending order, out[j] = s[lo[j]] where frac[j] == 0 and fp32(s[lo] + frac * (s[lo + 1] - s[lo])) otherwise, each fp64
        operation rounded on its own.  A NaN sample makes the Q outputs of its element NaN."""
        name, N, B = "ensemble_quantiles", int(N), int(B)
        if not isinstance(groups, (list, tuple)) or not 1 <= len(groups) <= FEED_GROUPS:
            raise ValueError(f"mmdyn_hip: {name}: between 1 and {FEED_GROUPS} groups, got "
                             f"{len(groups) if isinstance(groups, (list, tuple)) else type(groups).__name__}")
        if B < 1 or not 1 <= N <= QUANTILE_N_MAX:
            raise ValueError(f"mmdyn_hip: {name}: B = {B} must be positive and N = {N} lie in [1, {QUANTILE_N_MAX}]")
        if not isinstance(lo, (list, tuple)) or not isinstance(frac, (list, tuple)) or len(lo) != len(frac) or \
                not 1 <= len(lo) <= QUANTILES_MAX:
            raise ValueError(f"mmdyn_hip: {name}: lo and frac must be sequences of one length in [1, {QUANTILES_MAX}]")
        Q = len(lo)
        for j in range(Q):
            if isinstance(lo[j], bool) or not isinstance(lo[j], int) or not 0 <= lo[j] < N or not 0.0 <= float(frac[j]) < 1.0:
                raise ValueError(f"mmdyn_hip: {name}: quantile {j}: lo = {lo[j]!r} must be an int in [0, N={N}) and frac = "
                                 f"{frac[j]!r} lie in [0, 1)")
        like = groups[0]["src"]
        for g, grp in enumerate(groups):
            src, out = grp["src"], grp["out"]
            for t, rows, what in ((src, (N * B,), "src"), (out, (Q, B), "out")):
                if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < len(rows) or \
                        tuple(t.shape[:len(rows)]) != rows:
                    raise ValueError(f"mmdyn_hip: {name}: group {g}: {what} must be a contiguous fp32 tensor {list(rows)}[...], got "
                                     f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
            if src.numel() == 0 or tuple(src.shape[1:]) != tuple(out.shape[2:]) or src.device != like.device or out.device != like.device:
                raise ValueError(f"mmdyn_hip: {name}: group {g}: src {tuple(src.shape)} on {src.device} and out {tuple(out.shape)} on "
                                 f"{out.device} must share a non-empty row shape and the device {like.device}")
            if max(N, Q) * (src.numel() // N) >= 1 << 31:
                raise ValueError(f"mmdyn_hip: {name}: group {g}: {max(N, Q) * (src.numel() // N)} elements reach 2^31")
        for g, grp in enumerate(groups):
            for h, other in enumerate(groups):
                if self._touch(grp["out"], other["src"]) or (h != g and self._touch(grp["out"], other["out"])):
                    raise ValueError(f"mmdyn_hip: {name}: the out of group {g} overlaps a tensor of group {h}")
        arg = QuantileGroups()
        for g, grp in enumerate(groups):
            arg.src[g], arg.out[g] = _ptr(grp["src"]), _ptr(grp["out"])
            arg.row_len[g], arg.logits[g] = grp["src"].numel() // (N * B), int(bool(grp["logits"]))
        for j in range(Q):
            arg.lo[j], arg.frac[j] = lo[j], float(frac[j])
        check(self.lib.mmdyn_ensemble_quantiles(ctypes.addressof(arg), len(groups), Q, N, B, _stream()), "mmdyn_ensemble_quantiles")

    # ---- importance-weighted K-sample bound (evaluation only) ----
    @staticmethod
    def _iw_tables(name, *specs):
        """Pointers of contiguous GPU tables, each given as (tensor | None, shape, what, dtype): every shape and dtype is checked
        (ValueError) before the first pointer is taken (a CPU tensor: RuntimeError); None stays None."""
        HipBackend._check_tables(name, *specs)
        return [_ptr(t, dtype) for t, _, _, dtype in specs]

    @staticmethod
    def _check_tables(name, *specs):
        """The shape / dtype / contiguity half of :meth:`_iw_tables`: ValueError, no pointer is taken."""
        for t, shape, what, dtype in specs:
            if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous()):
                raise ValueError(f"mmdyn_hip: {name}: {what} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got "
                                 f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")

    def iw_latent(self, mu, lv, eps_noise, z, ratio, K, B, L):
        """mu / lv: fp32 [B, L] rows (may be column views of a fused heads output: unit inner stride, one row stride for both);
        eps_noise: fp32 [K][B][L], read; z: fp32 [K][B][L] = eps * exp(lv / 2) + mu, written; ratio: fp64 [K][B] =
        sum_L 0.5 * (z^2 - eps^2 - lv), written (no zeroing needed)."""
        K, B, L = int(K), int(B), int(L)
        if K < 1 or B < 1 or L < 1:
            raise ValueError(f"mmdyn_iw_latent: K = {K}, B = {B}, L = {L} must all be positive")
        for t, what in ((mu, "mu"), (lv, "lv")):
            if t.dtype != torch.float32 or tuple(t.shape) != (B, L) or t.stride(1) != 1:
                raise ValueError(f"mmdyn_iw_latent: {what} must be fp32 [B={B}, L={L}] with unit inner stride, got {t.dtype} "
                                 f"{tuple(t.shape)}")
        ld = mu.stride(0) if B > 1 else max(mu.stride(0), L)
        if (B > 1 and lv.stride(0) != ld) or ld < L:
            raise ValueError(f"mmdyn_iw_latent: mu and lv must share one row stride >= L (got {mu.stride(0)} and {lv.stride(0)})")
        f32, f64 = torch.float32, torch.float64
        e, zp, rp = self._iw_tables("iw_latent", (eps_noise, (K, B, L), "eps", f32), (z, (K, B, L), "z", f32), (ratio, (K, B), "ratio", f64))
        if not (mu.is_cuda and lv.is_cuda):
            raise RuntimeError("mmdyn_hip: the HIP path needs GPU tensors (got a CPU tensor); there is no CPU fallback")
        check(self.lib.mmdyn_iw_latent(mu.data_ptr(), lv.data_ptr(), ld, e, zp, rp, K, B, L, _stream()), "mmdyn_iw_latent")

    def iw_assemble_rows(self, bce_rows, mse_rows, ratio, tavail, out, ess, log_w, K, B, pose_multiplier, kl_weight=1.0,
                         kl_weight_dev=None):
        """bce_rows: fp64 [n_bce <= 2][K][B] (visual, tactile) or None; mse_rows: fp64 [K][B] or None; ratio: fp64 [K][B]; tavail:
        the target-availability table (uint8 [B][4]) or None; out: fp32 [B] = -(logsumexp_k log_w - log K) with log_w[k][b] =
        -(bce + pose_multiplier * mse) - kl_weight * ratio; ess: fp32 [B] or None; log_w: fp64 [K][B] or None.  The K table entries
        of a (row, term) whose target is absent are overwritten with 0."""
        K, B = int(K), int(B)
        if K < 1 or B < 1:
            raise ValueError(f"mmdyn_iw_assemble_rows: K = {K} and B = {B} must be positive")
        n_bce = 0
        if bce_rows is not None:
            if bce_rows.dim() != 3 or not 1 <= bce_rows.shape[0] <= 2:
                raise ValueError(f"mmdyn_iw_assemble_rows: bce_rows must be fp64 [1 or 2][K={K}][B={B}], got {tuple(bce_rows.shape)}")
            n_bce = bce_rows.shape[0]
        name, f32, f64 = "iw_assemble_rows", torch.float32, torch.float64
        tp = self._avail(tavail, B, name, out)
        bp, mp, rp, op, ep, lp = self._iw_tables(name, (bce_rows, (n_bce, K, B), "bce_rows", f64), (mse_rows, (K, B), "mse_rows", f64),
                                                 (ratio, (K, B), "ratio", f64), (out, (B,), "out", f32), (ess, (B,), "ess", f32),
                                                 (log_w, (K, B), "log_w", f64))
        check(self.lib.mmdyn_iw_assemble_rows(bp, mp, rp, tp, op, ep, lp, n_bce, K, B,
                                              float(pose_multiplier), float(kl_weight), _ptr(kl_weight_dev), _stream()),
              "mmdyn_iw_assemble_rows")

    # ---- weighted per-sample ELBO: the gradient seeds with a per-sample scale ----
    @staticmethod
    def _weights(w, B, name):
        """Pointer of a per-sample weight vector: fp32 [B], contiguous."""
        if w is None or w.dtype != torch.float32 or w.numel() != B or not w.is_contiguous():
            raise ValueError(f"mmdyn_hip: {name}: the weights must be a contiguous fp32 vector of B={B} elements")
        return _ptr(w)

    def tconv_out3_bn_bce_rows_grad(self, y, mean, rstd, gamma, beta, w, logits, logits_group, target, dlogit, w_rec, loss_rows,
                                    slot_of_group, grad_scale, G, Bg, Hi, Wi, mask=None, mask_channels=1, unmasked_rows=None):
        """tconv_out3_bn_bce_rows with the gradient output: dlogit = ((sigmoid - t) * grad_scale) * w_rec[b]; the rows stay
        unweighted."""
        py, y16 = _aptr(y)
        name = "tconv_out3_bn_bce_rows_grad"
        if len(slot_of_group) != G or tuple(target.shape) != (Bg, 3, 2 * Hi, 2 * Wi):
            raise ValueError(f"mmdyn_hip: {name}: one slot per group and a [Bg][3][2Hi][2Wi] target")
        if logits is not None and logits.numel() != (G if logits_group < 0 else 1) * Bg * 3 * 4 * Hi * Wi:
            raise ValueError(f"mmdyn_hip: {name}: logits buffer of the wrong size")
        if dlogit is None or dlogit.numel() != G * Bg * 3 * 4 * Hi * Wi:
            raise ValueError(f"mmdyn_hip: {name}: dlogit buffer of the wrong size")
        if mask is not None and tuple(mask.shape) != (Bg, mask_channels, 2 * Hi, 2 * Wi):
            raise ValueError(f"mmdyn_hip: {name}: mask {tuple(mask.shape)} is not [Bg][{mask_channels}][2Hi][2Wi]")
        n_slots = self._row_slots(loss_rows, Bg, name)
        if unmasked_rows is not None and self._row_slots(unmasked_rows, Bg, name) != n_slots:
            raise ValueError(f"mmdyn_hip: {name}: unmasked_rows and loss_rows differ in shape")
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        check(self.lib.mmdyn_tconv_out3_bn_bce_rows_grad(py, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(w), _ptr(logits),
                                                         int(logits_group), _ptr(target), _ptr(mask), int(mask_channels),
                                                         _ptr(dlogit), self._weights(w_rec, Bg, name),
                                                         _ptr(loss_rows, torch.float64), _ptr(unmasked_rows, torch.float64),
                                                         ctypes.addressof(slots), n_slots, float(grad_scale), G, Bg, Hi, Wi, y16,
                                                         _stream()), "mmdyn_" + name)

    def bce_logits_rows_groups_grad(self, logits, target, dlogit, w_rec, rows_out, slot_of_group, Bg, chw, grad_scale, mask=None,
                                    hw=0, mask_channels=1, unmasked_rows=None):
        """bce_logits_rows_groups with dlogit [G*Bg*chw] = ((sigmoid - t) * grad_scale) * w_rec[b] (zeros for a negative slot)."""
        G = len(slot_of_group)
        name = "bce_logits_rows_groups_grad"
        n_slots = self._row_slots(rows_out, Bg, name)
        if logits.numel() != G * Bg * chw or target.numel() != Bg * chw or dlogit is None or dlogit.numel() != G * Bg * chw:
            raise ValueError(f"mmdyn_{name}: logits / dlogit / target do not match [G={G}][Bg={Bg}][chw={chw}]")
        if mask is not None and (hw <= 0 or mask.numel() != Bg * mask_channels * hw):
            raise ValueError(f"mmdyn_{name}: mask of {mask.numel()} elements does not match [Bg={Bg}][{mask_channels}][hw={hw}]")
        if unmasked_rows is not None and self._row_slots(unmasked_rows, Bg, name) != n_slots:
            raise ValueError(f"mmdyn_{name}: unmasked_rows and rows_out differ in shape")
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        check(self.lib.mmdyn_bce_logits_rows_groups_grad(_ptr(logits), _ptr(target), _ptr(mask), int(mask_channels), _ptr(dlogit),
                                                         self._weights(w_rec, Bg, name), _ptr(rows_out, torch.float64),
                                                         _ptr(unmasked_rows, torch.float64), ctypes.addressof(slots), n_slots,
                                                         float(grad_scale), G, Bg, chw, hw, _stream()), "mmdyn_" + name)

    def mse_rows_groups_grad(self, r, t, dr, w_rec, rows_out, slot_of_group, Bg, n, grad_scale):
        """mse_rows_groups with dr [G*Bg*n] = (2 (r - t) * grad_scale) * w_rec[b]."""
        G = len(slot_of_group)
        name = "mse_rows_groups_grad"
        n_slots = self._row_slots(rows_out, Bg, name)
        if r.numel() != G * Bg * n or t.numel() != Bg * n or dr is None or dr.numel() != G * Bg * n:
            raise ValueError(f"mmdyn_{name}: r / dr / t do not match [G={G}][Bg={Bg}][n={n}]")
        slots = (ctypes.c_int * G)(*[int(s) for s in slot_of_group])
        check(self.lib.mmdyn_mse_rows_groups_grad(_ptr(r), _ptr(t), _ptr(dr), self._weights(w_rec, Bg, name),
                                                  _ptr(rows_out, torch.float64), ctypes.addressof(slots), n_slots, float(grad_scale),
                                                  G, Bg, n, _stream()), "mmdyn_" + name)

    def poe_bwd_weighted(self, passes, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale, w_kl, with_prior, P, B, L,
                         kl_weight_dev=None):
        """poe_bwd with the KL scale of row b = kl_scale * w_kl[b] (w_kl: fp32 [B])."""
        arr = self._passes(passes)
        check(self.lib.mmdyn_poe_bwd_weighted(ctypes.cast(arr, ctypes.c_void_p), _ptr(eps_noise), _ptr(mu), _ptr(logvar), _ptr(dz),
                                              _ptr(g_mu), _ptr(g_lv), float(kl_scale), self._weights(w_kl, B, "poe_bwd_weighted"),
                                              int(with_prior), P, B, L, _ptr(kl_weight_dev), _stream()), "mmdyn_poe_bwd_weighted")

    def reparam_bwd_weighted(self, mu, lv, eps_noise, dz, kl_scale, w_kl, dmu, dlv, B, L, ld):
        check(self.lib.mmdyn_reparam_bwd_weighted(mu.data_ptr(), lv.data_ptr(), _ptr(eps_noise), _ptr(dz), float(kl_scale),
                                                  self._weights(w_kl, B, "reparam_bwd_weighted"), dmu.data_ptr(), dlv.data_ptr(),
                                                  B, L, ld, _stream()), "mmdyn_reparam_bwd_weighted")

    def elbo_assemble_weighted(self, bce_rows, mse_rows, kl_rows, kl_sum, w, loss, wpartials, out, partials, w_sum_out, P, B,
                               kl_weight, pose_multiplier, kl_weight_dev=None, kl_mode=0):
        """loss [1] / wpartials [P]: the weighted scalar (1/B) sum_b w_b row_b and its per-pass parts; out [B] / partials [P][B]:
        the unweighted rows of elbo_assemble_rows; w_sum_out [B] (optional): filled with sum_b w_b.  Deterministic."""
        for t, n, what in ((bce_rows, P * B, "bce_rows"), (mse_rows, P * B, "mse_rows"), (kl_rows, P * B, "kl_rows"),
                           (kl_sum, P, "kl_sum"), (partials, P * B, "partials"), (out, B, "out"), (wpartials, P, "wpartials"),
                           (w_sum_out, B, "w_sum_out"), (loss, 1, "loss")):
            if t is not None and t.numel() < n:
                raise ValueError(f"mmdyn_elbo_assemble_weighted: {what} holds {t.numel()} elements, needs {n}")
        check(self.lib.mmdyn_elbo_assemble_weighted(_ptr(bce_rows, torch.float64), _ptr(mse_rows, torch.float64),
                                                    _ptr(kl_rows, torch.float64), _ptr(kl_sum, torch.float64),
                                                    self._weights(w, B, "elbo_assemble_weighted"), _ptr(loss), _ptr(wpartials),
                                                    _ptr(out), _ptr(partials), _ptr(w_sum_out), P, B, float(kl_weight),
                                                    float(pose_multiplier), _ptr(kl_weight_dev), int(kl_mode), _stream()),
              "mmdyn_elbo_assemble_weighted")

    # ---- the training step on a mixed-modality batch: input availability in the PoE, target availability in the loss ----
    def poe_bwd_avail_weighted(self, passes, avail, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale, w_kl, with_prior, P, B, L,
                               kl_weight_dev=None):
        """poe_bwd with the tables of poe_bwd_avail AND the row weights of poe_bwd_weighted."""
        name = "poe_bwd_avail_weighted"
        arr = self._passes(passes)
        tabs = self._avail_tables(avail, P, B, name, mu)
        check(self.lib.mmdyn_poe_bwd_avail_weighted(ctypes.cast(arr, ctypes.c_void_p), None if tabs is None else ctypes.addressof(tabs),
                                                    _ptr(eps_noise), _ptr(mu), _ptr(logvar), _ptr(dz), _ptr(g_mu), _ptr(g_lv),
                                                    float(kl_scale), self._weights(w_kl, B, name), int(with_prior), P, B, L,
                                                    _ptr(kl_weight_dev), _stream()), "mmdyn_" + name)

    def term_weights(self, tavail, w, w_term, B):
        """w_term [3][B] fp32: w_term[m][b] = tavail[b][m] != 0 ? (w[b], or 1 without w) : 0 -- the weight vectors of the visual,
        tactile and pose gradient seeds.  tavail: uint8 [B][4] or None (every target present); w: fp32 [B] or None."""
        name = "term_weights"
        if w_term is None or w_term.dtype != torch.float32 or tuple(w_term.shape) != (3, B) or not w_term.is_contiguous():
            raise ValueError(f"mmdyn_{name}: w_term must be a contiguous fp32 [3][B={B}] tensor")
        check(self.lib.mmdyn_term_weights(self._avail(tavail, B, name, w_term), None if w is None else self._weights(w, B, name),
                                          _ptr(w_term), B, _stream()), "mmdyn_" + name)

    def elbo_assemble_avail_weighted(self, bce_v_rows, bce_t_rows, mse_rows, kl_rows, kl_sum, w, tavail, loss, wpartials, out, partials,
                                     w_sum_out, present, term_sums, P, B, kl_weight, pose_multiplier, kl_weight_dev=None, kl_mode=0):
        """elbo_assemble_weighted with one fp64 [P][B] table per term (visual BCE, tactile BCE, pose MSE; any None = 0) and the
        target-availability table ``tavail`` (uint8 [B][4] or None): an absent (row, term) is selected out of every sum and its table
        entries are overwritten with 0.  w None = 1.  present fp64 [3] / term_sums fp64 [3][P] (optional): the number of rows that
        hold each target, and each term's unweighted per-pass sum over them.  Deterministic."""
        name = "elbo_assemble_avail_weighted"
        for t, n, what in ((bce_v_rows, P * B, "bce_v_rows"), (bce_t_rows, P * B, "bce_t_rows"), (mse_rows, P * B, "mse_rows"),
                           (kl_rows, P * B, "kl_rows"), (kl_sum, P, "kl_sum"), (partials, P * B, "partials"), (out, B, "out"),
                           (wpartials, P, "wpartials"), (w_sum_out, B, "w_sum_out"), (loss, 1, "loss"), (present, 3, "present"),
                           (term_sums, 3 * P, "term_sums")):
            if t is not None and t.numel() < n:
                raise ValueError(f"mmdyn_{name}: {what} holds {t.numel()} elements, needs {n}")
        f64 = torch.float64
        check(self.lib.mmdyn_elbo_assemble_avail_weighted(_ptr(bce_v_rows, f64), _ptr(bce_t_rows, f64), _ptr(mse_rows, f64),
                                                          _ptr(kl_rows, f64), _ptr(kl_sum, f64),
                                                          None if w is None else self._weights(w, B, name),
                                                          self._avail(tavail, B, name, loss), _ptr(loss), _ptr(wpartials), _ptr(out),
                                                          _ptr(partials), _ptr(w_sum_out), _ptr(present, f64), _ptr(term_sums, f64),
                                                          P, B, float(kl_weight), float(pose_multiplier), _ptr(kl_weight_dev),
                                                          int(kl_mode), _stream()), "mmdyn_" + name)

    def adam_step(self, p, g, m, v, state, lr, beta1, beta2, eps, grad_scale, guarded=False):
        """guarded: ``state`` has six doubles and a gradient holding inf / NaN skips the step (counted in state[4])."""
        if guarded and state.numel() < 6:
            raise ValueError("mmdyn_hip: the guarded Adam step keeps six doubles of state")
        fn = self.lib.mmdyn_adam_step_guarded if guarded else self.lib.mmdyn_adam_step
        check(fn(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(state, torch.float64), p.numel(), lr, beta1, beta2, eps, grad_scale,
                 _stream()), "mmdyn_adam_step")


    def sgd_step(self, p, g, buf, lr, momentum, weight_decay, grad_scale, first):
        check(self.lib.mmdyn_sgd_step(_ptr(p), _ptr(g), _ptr(buf), p.numel(), lr, momentum, weight_decay, grad_scale,
                                      int(first), _stream()), "mmdyn_sgd_step")

    # ---- clipping by the global L2 norm: clip = fp64 [4] on the device {sum of squares, norm, coefficient, clipped steps} ----
    def grad_sumsq_blocks(self, n):
        """Doubles of workspace ``grad_sumsq`` wants for a buffer of ``n`` elements (a function of n alone)."""
        return self.lib.mmdyn_grad_sumsq_blocks(int(n))

    def grad_sumsq(self, g, partials, clip, accumulate=False):
        """clip[0] = sum g^2 in fp64 (``accumulate``: added to clip[0]), deterministic.  g: fp32, any number of elements, 4-byte
        aligned (a view that starts inside a buffer is fine); partials: fp64 workspace of ``grad_sumsq_blocks(g.numel())``."""
        _check_clip(clip, "grad_sumsq")
        need = self.grad_sumsq_blocks(g.numel())
        if partials is None or partials.dtype != torch.float64 or partials.numel() < need:
            raise ValueError(f"mmdyn_grad_sumsq: partials must be an fp64 workspace of at least {need} values for {g.numel()} elements")
        check(self.lib.mmdyn_grad_sumsq(_ptr(g), g.numel(), _ptr(partials, torch.float64), _ptr(clip, torch.float64),
                                        int(bool(accumulate)), _stream()), "mmdyn_grad_sumsq")

    def grad_clip_coef(self, clip, grad_scale, max_norm):
        """clip[1] = |grad_scale| sqrt(clip[0]), clip[2] = min(1, max_norm / (clip[1] + 1e-6)), clip[3] += 1 when that clips."""
        _check_clip(clip, "grad_clip_coef")
        max_norm = check_max_norm(max_norm, "max_norm")
        check(self.lib.mmdyn_grad_clip_coef(_ptr(clip, torch.float64), grad_scale, max_norm, _stream()), "mmdyn_grad_clip_coef")

    def adam_step_clipped(self, p, g, m, v, state, clip, lr, beta1, beta2, eps, grad_scale, guarded=False):
        """``adam_step`` with the gradient factor float32(grad_scale * clip[2]).  guarded: six doubles of state; the step is skipped
        and counted in state[4] when the norm in clip[1] is not finite."""
        _check_clip(clip, "adam_step_clipped")
        if state.numel() < (6 if guarded else 3):
            raise ValueError("mmdyn_hip: the guarded Adam step keeps six doubles of state" if guarded else
                             "mmdyn_hip: the Adam step keeps three doubles of state")
        check(self.lib.mmdyn_adam_step_clipped(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(state, torch.float64),
                                               _ptr(clip, torch.float64), p.numel(), lr, beta1, beta2, eps, grad_scale,
                                               int(bool(guarded)), _stream()), "mmdyn_adam_step_clipped")

    def sgd_step_clipped(self, p, g, buf, clip, lr, momentum, weight_decay, grad_scale, first):
        _check_clip(clip, "sgd_step_clipped")
        check(self.lib.mmdyn_sgd_step_clipped(_ptr(p), _ptr(g), _ptr(buf), _ptr(clip, torch.float64), p.numel(), lr, momentum,
                                              weight_decay, grad_scale, int(first), _stream()), "mmdyn_sgd_step_clipped")

    # ---- EMA of the parameters: ema_state = fp64 [4] on the device {updates done, decay, 1 - d_n, warm-up flag} (new_ema_state) ----
    def ema_tick(self, ema_state, adam_state=None):
        """One update of the EMA state: ema_state[2] = 1 - d_n, ema_state[0] += 1.  ``adam_state``: the six-double state of a guarded
        Adam step that has run; when it skipped, the tick changes nothing."""
        _check_ema(None, None, ema_state, "ema_tick")
        if adam_state is not None and adam_state.numel() < 6:
            raise ValueError("mmdyn_hip: the guarded Adam step keeps six doubles of state")
        check(self.lib.mmdyn_ema_tick(_ptr(ema_state, torch.float64), _ptr(adam_state, torch.float64), _stream()), "mmdyn_ema_tick")

    def ema_update(self, ema, p, ema_state):
        """ema = fmaf(float32(ema_state[2]), p - ema, ema) per element.  fp32, 4-byte aligned views are fine."""
        _check_ema(ema, p, ema_state, "ema_update")
        check(self.lib.mmdyn_ema_update(_ptr(ema), _ptr(p), _ptr(ema_state, torch.float64), p.numel(), _stream()), "mmdyn_ema_update")

    def adam_step_ema(self, p, g, m, v, ema, state, clip, ema_state, lr, beta1, beta2, eps, grad_scale, guarded=False):
        """``adam_step`` (``clip`` None) or ``adam_step_clipped`` that also moves ``ema`` towards the new parameters in the same pass:
        the bits of that step followed by ``ema_tick`` + ``ema_update``.  A step the guard skips leaves ``ema`` and ``ema_state``
        untouched."""
        _check_ema(ema, p, ema_state, "adam_step_ema")
        if clip is not None:
            _check_clip(clip, "adam_step_ema")
        if state.numel() < (6 if guarded else 3):
            raise ValueError("mmdyn_hip: the guarded Adam step keeps six doubles of state" if guarded else
                             "mmdyn_hip: the Adam step keeps three doubles of state")
        check(self.lib.mmdyn_adam_step_ema(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), _ptr(state, torch.float64),
                                           _ptr(clip, torch.float64), _ptr(ema_state, torch.float64), p.numel(), lr, beta1, beta2,
                                           eps, grad_scale, int(bool(guarded)), _stream()), "mmdyn_adam_step_ema")

    # ---- image grids of the epoch log (problems.py:588-603: slices, cat, make_grid and the writer's uint8 conversion) ----
    def image_grid(self, srcs, take, nrow, logits, padding=2, out=None):
        """The uint8 [Hg, Wg, 3] grid (HWC: a PNG's scanlines) of the first ``take`` images of each source -- ``srcs``: one fp32
        [n, C, H, W] tensor, or a list / tuple of one or two of one C / H / W --, ``nrow`` tiles per row, laid out as
        ``torchvision.utils.make_grid(..., nrow, padding)``; ``logits``: the sources are decoder logits and go through the sigmoid.
        One launch on the current stream; ``out`` is allocated on the sources' device when None."""
        srcs = check_grid_sources(srcs, take, nrow, padding)
        n = [int(s.shape[0]) for s in srcs]
        C, H, W = (int(d) for d in srcs[0].shape[1:])
        shape = grid_shape(sum(min(k, take) for k in n), H, W, nrow, padding) + (3,)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=srcs[0].device)
        else:
            check_grid_out(out, shape, srcs[0].device)
        check(self.lib.mmdyn_image_grid_u8(_ptr(srcs[0]), _ptr(srcs[1]) if len(srcs) > 1 else None, _ptr(out, torch.uint8), n[0],
                                           n[1] if len(srcs) > 1 else 0, int(take), C, H, W, int(nrow), int(padding),
                                           int(bool(logits)), _stream()), "mmdyn_image_grid_u8")
        return out


    # ---- image decode (uint8 HWC frames in HBM -> float32 CHW) ----
    def resize_plan(self, in_size, out_size, device):
        """(bounds int32 [out][2], coeffs int32 [out][ksize]) of Pillow's 8-bit bilinear resampler, on ``device``."""
        ks = self.lib.mmdyn_resize_ksize(in_size, out_size)
        check(min(ks, 0), "mmdyn_resize_ksize")
        bounds = torch.empty(out_size, 2, dtype=torch.int32)
        coeffs = torch.empty(out_size, ks, dtype=torch.int32)
        check(min(self.lib.mmdyn_resize_plan(in_size, out_size, bounds.data_ptr(), coeffs.data_ptr()), 0),
              "mmdyn_resize_plan")
        return bounds.to(device), coeffs.to(device)

    def resize_u8_to_chw_f32(self, src, index, dst, n_out, Hin, Win, Hout, Wout, xb, xk, yb, yk):
        I32 = torch.int32
        check(self.lib.mmdyn_resize_u8_to_chw_f32(_ptr(src, torch.uint8), _ptr(index, I32), _ptr(dst), n_out, Hin, Win,
                                                  Hout, Wout, _ptr(xb, I32), _ptr(xk, I32), _ptr(yb, I32),
                                                  _ptr(yk, I32), _stream()), "mmdyn_resize_u8_to_chw_f32")


B = HipBackend()


def set_backend(b):
    """Test hook only (tests/emu_backend.py): swap the object that executes the ops."""
    global B
    old, B = B, b
    return old


def backend_op(name):
    """The op ``name`` of the active backend.  A backend that does not have it (one written before the op was added) is an error
    that names the op, never a fallback: a ``RuntimeError``, which is also what autograd raises for a result without a graph."""
    op = getattr(B, name, None)
    if op is None:
        raise RuntimeError(f"the active backend ({type(B).__name__}) has no op {name!r}; there is no fallback path")
    return op
