"""Hand-scheduled cnn-mvae training / evaluation step (the throughput path).

Computes exactly what the reference's ``Reconstruction._evaluate_mvae`` + ``loss.backward()`` +
``Adam.step()`` compute (/root/reference/mmdyn/pytorch/problems/problems.py:473-546, 148-156) -- the sum
over the 3 (or 7, with pose) modality-subset ELBOs and its gradient -- but restructured for the GPU:

  * each image-encoder trunk runs ONCE per step (its 4 reference runs are bit-identical up to the
    dropout mask); only dropout -> heads is evaluated per pass, batched as 4B rows;
  * the 4 live passes of each image decoder are one batch of 4 groups with per-group BatchNorm
    statistics; decoder outputs the reference computes and discards ("dead" passes) are not computed;
  * PoE + reparametrisation + KL of all passes is one kernel; BCE/MSE produce their gradients in the
    same pass; the backward is an explicit reverse schedule writing straight into one flat gradient
    buffer, which is what RCCL all-reduces (three buckets, overlapped with the remaining backward)
    before the fused Adam kernel.

Loss value, every partial ELBO and every parameter gradient equal the reference's up to fp32
summation order (tests/test_engine_*.py).  BatchNorm running statistics: encoder buffers receive the same
4 EMA updates as in the reference; decoder buffers receive the live passes' updates only (the
reference also folds in the discarded passes) unless ``exact_running_stats=True``.
"""
import collections.abc
import math
import numbers
import os
import torch

from . import layers, ops
from .models.shapes import DROPOUT_P

# A/B switches of bench.py (measurements only; the product runs with all of them on)
FUSED_BCE = True       # the BCE term in the last decoder layer's epilogue
COPY_MANY = True       # the batch moved into the static buffers by one launch

SUBSETS_POSE = [(1, 1, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1)]
SUBSETS_NOPOSE = SUBSETS_POSE[:3]
# "fp32x3": fp32 storage and fp32 results like "fp32"; the GEMM launches that gain from it run on the bf16 matrix cores through the
# exact three-term split of their fp32 operands (ops.HipBackend.fp32_split, csrc/igemm_nt.hip X3) -- error against fp64 no larger
# than the native fp32 matrix cores', six bf16 MFMAs per product at 16x the fp32 rate
PRECISIONS = ("fp32", "fp32x3", "bf16", "bf16s", "fp16", "fp16s")


def _select_precision(precision):
    """Select an engine precision on the active backend; returns the previous (precision, fp32_split) pair."""
    prev = (getattr(ops.B, "precision", "fp32"), getattr(ops.B, "fp32_split", False))
    ops.B.precision = "fp32" if precision == "fp32x3" else precision
    ops.B.fp32_split = precision == "fp32x3"
    return prev


def _restore_precision(prev):
    ops.B.precision, ops.B.fp32_split = prev


def act_dtype(precision):
    """Storage type of the convolution-level activations (and their gradients) of a precision mode."""
    return {"bf16s": torch.bfloat16, "fp16s": torch.float16}.get(precision, torch.float32)


def w_dtype(precision):
    """Type the packed GEMM operands (weights) are written in: the matrix cores' operand type where the storage is 16-bit
    anyway ("bf16" packs bf16 too: the kernels round fp32 weights to bf16 on their way in, packing does it once)."""
    return {"bf16": torch.bfloat16, "bf16s": torch.bfloat16, "fp16s": torch.float16}.get(precision, torch.float32)

HEAD_GROUP_ORDER = ("visual_encoder", "tactile_encoder", "pose_encoder")    # groups of the grouped heads launches

_PREFIX_ORDER = ["pose_decoder", "visual_decoder", "tactile_decoder",         # bucket 0: ready first
                 "heads", "pose_encoder", "encoder_fc",                      # bucket 1: heads, pose encoder and the image
                 #                      encoders' FC layer (two thirds of the encoder parameters, first in their backward)
                 "visual_encoder", "tactile_encoder"]                        # bucket 2: the encoder conv stacks, ready last


def _align4(n):
    return (n + 3) // 4 * 4


class FlatParams:
    """All parameters (and their gradients) as views into two flat fp32 buffers, ordered by the time their
    gradient becomes available in the backward schedule (so contiguous slices are all-reduce buckets)."""

    def __init__(self, model):
        named = dict(model.named_parameters())
        # the two heads of an encoder are ONE fused GEMM ([means | log_var] rows): keeping their weights adjacent (and
        # their biases adjacent) in the flat buffers lets the backward write both gradients as one [2L][K] / [2L] block
        # ... and the heads of ALL encoders are one GROUPED launch each way (layers.heads_*_grouped): their weights follow
        # one another in group order (visual, tactile, pose) -- [G][2L][K] --, their biases behind them
        rank = {"linear_means.weight": 0, "linear_log_var.weight": 1, "linear_means.bias": 2, "linear_log_var.bias": 3}
        enc_order = {p: i for i, p in enumerate(HEAD_GROUP_ORDER)}
        heads = sorted((k for k in named if ".linear_" in k),
                       key=lambda k: (rank[k.split(".", 1)[1]] >= 2, enc_order.get(k.split(".", 1)[0], 99), k.split(".", 1)[0],
                                      rank[k.split(".", 1)[1]]))
        groups = {p: [] for p in _PREFIX_ORDER}
        groups["heads"] = list(heads)
        for k in named:
            if k in heads:
                continue
            elif k.split(".", 1)[0] in ("visual_encoder", "tactile_encoder") and ".fc_net." in k:
                groups["encoder_fc"].append(k)
            else:
                groups[k.split(".", 1)[0]].append(k)
        self.order, self.offsets, self.bucket_bounds = [], {}, []
        off = 0
        marks = {"tactile_decoder": None, "encoder_fc": None, "tactile_encoder": None}
        for g in _PREFIX_ORDER:
            for k in groups[g]:
                self.order.append(k)
                self.offsets[k] = off
                off = _align4(off + named[k].numel())
            if g in marks:
                self.bucket_bounds.append(off)
        self.total = off
        dev = next(model.parameters()).device
        self.flat = torch.zeros(self.total, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(self.total, device=dev, dtype=torch.float32)
        self.P, self.G = {}, {}
        for k in self.order:
            p = named[k]
            o, n = self.offsets[k], p.numel()
            self.flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)
            self.P[k], self.G[k] = p.data, p.grad
        self.model = model

    def still_attached(self):
        named = dict(self.model.named_parameters())
        k = self.order[0]
        return named[k].data_ptr() == self.P[k].data_ptr()

    def fused_heads_grad(self, prefix):
        """(gW [2L][K], gb [2L]) views of the flat gradient buffer covering linear_means | linear_log_var of ``prefix``, or
        None when the two are not adjacent there."""
        kw = [f"{prefix}.linear_means.weight", f"{prefix}.linear_log_var.weight"]
        kb = [f"{prefix}.linear_means.bias", f"{prefix}.linear_log_var.bias"]
        L, K = self.P[kw[0]].shape
        if self.offsets[kw[1]] != self.offsets[kw[0]] + L * K or self.offsets[kb[1]] != self.offsets[kb[0]] + L:
            return None
        ow, ob = self.offsets[kw[0]], self.offsets[kb[0]]
        return self.grad[ow:ow + 2 * L * K].view(2 * L, K), self.grad[ob:ob + 2 * L]

    def grouped_heads_grad(self, prefixes):
        """(gW_all [G*2L][K], [gb_g [2L]]) views of the flat gradient buffer covering the heads of ``prefixes`` in that
        order, or None when they are not laid out [G][2L][K] there (unequal head shapes)."""
        views = [self.fused_heads_grad(p) for p in prefixes]
        if any(v is None for v in views):
            return None
        L, K = self.P[f"{prefixes[0]}.linear_means.weight"].shape
        o0 = self.offsets[f"{prefixes[0]}.linear_means.weight"]
        for g, p in enumerate(prefixes):
            if tuple(self.P[f"{p}.linear_means.weight"].shape) != (L, K) or \
                    self.offsets[f"{p}.linear_means.weight"] != o0 + g * 2 * L * K:
                return None
        G = len(prefixes)
        return self.grad[o0:o0 + G * 2 * L * K].view(G * 2 * L, K), [v[1] for v in views]

    def sub(self, prefix, which="P"):
        src = self.P if which == "P" else self.G
        return {k[len(prefix) + 1:]: v for k, v in src.items() if k.startswith(prefix + ".")}


class _Bf16Bucket:
    """Handle of one gradient bucket that travels in bf16: ``wait()`` orders the current stream behind the all-reduce (like
    the Work it wraps) and widens the reduced bucket back into the fp32 gradient buffer there."""

    def __init__(self, work, engine, lo, hi):
        self.work, self.engine, self.lo, self.hi = work, engine, lo, hi

    def wait(self):
        self.work.wait()
        e = self.engine
        ops.B.cast_bf16_to_f32(e._grad16[self.lo:self.hi], e.params.grad[self.lo:self.hi])

    def is_completed(self):
        return self.work.is_completed()


class _Lanes:
    """Two side streams for the independent visual / tactile halves of the schedule (HIP streams on the GPU,
    no-ops on the CPU emulation).  Every fork starts from the main stream's current point and every join
    returns to it, so buffers handed between lanes are ordered by events, never by luck."""

    def __init__(self, device, enabled=True):
        self.on = enabled and device.type == "cuda"
        if device.type == "cuda":        # (the graph path replays its lane graphs on these even when eager launches stay on one stream)
            # (LAB, MMDYN_LANE_PRIO=<p>: the two lanes as priority-p streams -- -1 = high -- next to default-priority weight-gradient streams)
            prio = int(os.environ.get("MMDYN_LANE_PRIO", "0"))
            self.side = [torch.cuda.Stream(device=device, priority=prio), torch.cuda.Stream(device=device, priority=prio)]

    def fork(self):
        if self.on:
            ev = torch.cuda.current_stream().record_event()
            for s in self.side:
                s.wait_event(ev)

    def lane(self, i):
        import contextlib

        @contextlib.contextmanager
        def ctx():
            prev, layers.CUR_LANE = layers.CUR_LANE, i
            try:
                if self.on:
                    with torch.cuda.stream(self.side[i]):
                        yield
                else:
                    yield
            finally:
                layers.CUR_LANE = prev
        return ctx()

    def join(self):
        if self.on:
            main = torch.cuda.current_stream()
            for s in self.side:
                main.wait_event(s.record_event())


def _with_precision(fn):
    """Run a step method with the engine's matrix-core precision selected on the active backend."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        prev_sync, prev_act, prev_w = layers.SYNC, layers.ACT_DTYPE, layers.W_DTYPE
        prev = _select_precision(self.precision)
        layers.SYNC = self._sync
        layers.ACT_DTYPE = act_dtype(self.precision)
        layers.W_DTYPE = w_dtype(self.precision)
        try:
            return fn(self, *a, **k)
        finally:
            _restore_precision(prev)
            layers.SYNC = prev_sync
            layers.ACT_DTYPE = prev_act
            layers.W_DTYPE = prev_w
    return wrapped


class _AvailTables:
    """The two availability tables of a mixed-modality step as the kernels take them (uint8 [B][4], models.functional.
    availability_table): ``inp`` -- which experts a row's posterior holds; ``tgt`` -- which reconstruction terms of a row count
    (the same tensor as ``inp`` when no target table was given).  Either may be None: every row holds everything."""
    __slots__ = ("inp", "tgt")

    def __init__(self, inp, tgt):
        self.inp, self.tgt = inp, tgt

    def clone(self):
        inp = None if self.inp is None else self.inp.clone()
        return _AvailTables(inp, inp if self.tgt is self.inp else self.tgt.clone())

    def pairs(self, src):
        """(dst, src) copies that move the contents of ``src`` (tables of the same presence) into these."""
        out = [] if self.inp is None else [(self.inp, src.inp)]
        return out + ([(self.tgt, src.tgt)] if (self.tgt is not None and self.tgt is not self.inp) else [])


class MVAEStep:
    """Fused train / eval step for an :class:`mmdyn_hip.models.MVAE` on one GPU (one rank)."""

    def __init__(self, model, lr=1e-3, pose_multiplier=1000.0, betas=(0.9, 0.999), eps=1e-8, noise=None,
                 process_group=None, world_size=1, two_lanes=True, precision="fp32x3", exact_running_stats=False, sync_bn=False,
                 defer_wgrad=None, grad_reduce_bf16=None, group_heads=True, keep_logits=False, max_grad_norm=None,
                 ema_decay=None, ema_warmup=False):
        # --conditional (vae.py:231-237, 286-291): the condition joins the 512 features in front of the image encoders' heads
        # and the latent in front of the image decoders' first layer; the pose MLPs are built unconditional (vae.py:117-123)
        self.conditional = bool(getattr(model, "conditional", False))
        # categorical conditions (vae.py:337-344): class indices [B]; the join kernel writes the one-hot rows and ORs bit 0 into
        # this engine-owned word for an index outside [0, condition_dim) -- cleared by the step's pre-phase (inside the captured
        # region), read by check_condition()
        self.categorical = self.conditional and bool(getattr(model, "categorical_conditions", False))
        self._bad_index = None
        # False (default): the image decoders' logits are materialised only for the pass whose reconstruction the caller receives
        # (outputs['recon_x'] = the joint pass: problems.py:537-545) -- the BCE term and dlogits come out of the last layer's
        # epilogue.  True: the logits of every live pass are written as well (self.last["logits_v" / "logits_t"])
        self.keep_logits = bool(keep_logits)
        if precision not in PRECISIONS:
            raise ValueError("precision must be 'fp32x3' (default: fp32 storage and results, the GEMMs on the bf16 matrix cores "
                             "through the exact three-term operand split), 'fp32' (the native fp32 matrix cores), 'bf16s' (bf16 activation storage + "
                             "bf16 matrix cores, fp32 accumulate / master weights: BASELINE configs[2]), 'bf16' (bf16 matrix-core "
                             "operands only, fp32 storage), 'fp16' (fp16 matrix-core operands, fp32 accumulate / storage: "
                             "BASELINE configs[4]) or 'fp16s' (fp16 + fp16 activation storage)")
        self.precision = precision
        # Loss scale of the fp16 modes: every loss gradient entering the backward (BCE / MSE / KL) is multiplied by
        # 4 * B and Adam divides it out again (the backward is linear in the loss gradient, BatchNorm included).  Unscaled,
        # dlogit is (sigmoid - t) / B and the KL gradient kl_w / B * ...: at B = 256 most of that signal sits below fp16's
        # smallest normal (6.1e-5) once it has passed a few layers and is rounded away on its way into the matrix cores.
        # Scaled, dlogit = 4 (sigmoid - t) whatever the batch; the largest operand is the pose gradient 8000 * |error|
        # (fp16 maximum 65504: pose targets and predictions live in [0, 1]).  ``params.grad`` holds the scaled gradients
        # between backward() and optimizer_step(): divide by ``loss_scale`` to read them.  Set per batch in _begin()
        # (4 * B * (64 / image side)^2: see there); data-parallel ranks must run equal local batches in these modes (bench.py
        # does), the all-reduce adds the ranks.  The scale is static; what a static scale cannot rule out -- an overflow to
        # inf somewhere in the backward -- is caught by the guarded Adam step (mmdyn_adam_step_guarded): such a step is
        # skipped, counted in ``skipped_steps``, and leaves parameters and moments as they were.
        self._scale_per_sample = 4.0 if precision in ("fp16", "fp16s") else 0.0
        # The decoders' weight-gradient GEMMs (nothing on the backward chain reads them) are queued during the decoder
        # backward and replayed as two more graphs during the encoder backward -- on the main stream since round 5 (_replay; rounds
        # 3-4: on two more streams).  None: the measured rule (tests/microbench/run_ab_defer_wgrad.sh, same box, alternating runs:
        # fp32 bs 256 +0.3 .. 0.9 % over three boxes, 128x128 fp32 7.0 -> 6.85 ms (+2 %), 256x256 fp32 +0.5 .. 5 %; the 16-bit
        # storage modes 0 .. -2 %) -- on in fp32 on one GPU.  Round 6, after the launch removals, measured again (same box, alternating,
        # profiles/r6/ab_defer_wgrad_16bit.txt): the 16-bit STORAGE modes gain 1.4-3.3 % at 64 and 128 pixels (bf16s bs 128 64.3 -> 65.8 k,
        # fp16s bs 128 63.7 -> 65.6 k, 128 px bf16s / fp16s +2.7 / +3.0 %) and nothing at 256 pixels (+-0.2 %); bf16 / fp16 on fp32
        # storage -0.2 ... +0.7 % at 64 pixels, fp16 at 256 pixels -1.3 % -- on for the storage modes below 256 pixels as well.
        # Data parallel: off, the decoders' gradient bucket would start its all-reduce a phase later.
        if defer_wgrad is None:
            side = int(getattr(getattr(model, "visual_decoder", None), "image_size", 64) or 64)
            defer_wgrad = process_group is None and (precision in ("fp32", "fp32x3") or (precision in ("bf16s", "fp16s") and side < 256))
        self.defer_wgrad = bool(defer_wgrad)
        self.loss_scale = 1.0
        # False (default): each image decoder runs only on the passes whose reconstruction enters the loss, so its
        # BatchNorm running buffers see 4 EMA updates per step (2 without pose) where the reference applies 7 (3).
        # True: the decoders also run on the passes the reference computes and discards, in pass order, with zero
        # loss gradient -- identical running_mean / running_var / num_batches_tracked, ~1.4x the step time.
        self.exact_running_stats = bool(exact_running_stats)
        # BatchNorm statistics over the global batch of the process group instead of each rank's shard (default:
        # local, like DistributedDataParallel).  Adds one small fp64 all-reduce per BatchNorm layer and direction and
        # With the RCCL backend the collectives are captured into the lanes' phase graphs (each lane on a communicator of its
        # own); with gloo (CPU tests) the step runs eagerly.
        if sync_bn and process_group is None:
            raise ValueError("sync_bn needs a process group")
        self._sync = None
        if sync_bn:
            import torch.distributed as dist
            ranks = dist.get_process_group_ranks(process_group)
            # one communicator per lane (see layers.SyncBN); created collectively: every rank constructs its engine
            lane_groups = [dist.new_group(ranks=ranks) for _ in range(2)]
            self._sync = layers.SyncBN(process_group, world_size, lane_groups)
            # collectives can be captured into HIP graphs with the RCCL backend only
            self._sync_graph_ok = dist.get_backend(process_group) == "nccl"
        self.model = model
        self.use_pose = bool(model._use_pose)
        self.L = model.latent_size
        self.subsets = SUBSETS_POSE if self.use_pose else SUBSETS_NOPOSE
        self.P = len(self.subsets)
        self.pass_v = [i for i, s in enumerate(self.subsets) if s[0]]
        self.pass_t = [i for i, s in enumerate(self.subsets) if s[1]]
        self.pass_p = [i for i, s in enumerate(self.subsets) if s[2]]
        self.lr, self.betas, self.eps = lr, betas, eps
        self.pose_multiplier = float(pose_multiplier)
        self.noise = noise
        self.pg, self.world = process_group, world_size
        self.params = FlatParams(model)
        dev = self.params.flat.device
        # Gradient buckets on the wire: fp32 by default; in the 16-bit storage modes the buckets are
        # rounded to bf16 in front of the all-reduce and widened back behind it (28.1 instead of 56.2 MB per step against a
        # ~2 ms step; bf16 rather than fp16 also for "fp16s": the loss-scaled gradients keep fp32's range).  Adam, its
        # moments and the master weights stay fp32.  ``grad_reduce_bf16`` overrides the rule.
        use16 = (precision in ("bf16s", "fp16s")) if grad_reduce_bf16 is None else bool(grad_reduce_bf16)
        self._grad16 = torch.empty(self.params.total, device=dev, dtype=torch.bfloat16) if (use16 and process_group is not None) else None
        self._warm_works = None      # list while the warm-up step in front of a graph capture runs: its collectives' Work handles
        self.adam_m = torch.zeros_like(self.params.flat)
        self.adam_v = torch.zeros_like(self.params.flat)
        self.adam_state = torch.zeros(6, dtype=torch.float64, device=dev)     # (six: the guarded step of the fp16 modes)
        # Clipping by the global L2 norm (None: off -- optimizer_step is the launches it has always been).  The norm is that of the
        # gradient Adam applies: the flat buffer after the all-reduce, times 1 / (world * loss scale) -- the averaged, unscaled
        # gradient whatever the loss scale of the fp16 modes, the same bits on every rank (each reduces the same buffer in the
        # same order, so no further collective).  Sum of squares, coefficient and the clipped Adam step are device-side and
        # allocate nothing, so the captured step holds them where it holds Adam.  inf: report the norm, never clip.  Fixed per
        # engine, so the capture key does not carry it.
        self.max_grad_norm = None if max_grad_norm is None else ops.check_max_norm(max_grad_norm, "max_grad_norm")
        self.clip = self._sumsq_ws = None       # clip: fp64 {sum of squares, norm, coefficient, clipped steps}
        if self.max_grad_norm is not None:
            self.clip = torch.zeros(4, dtype=torch.float64, device=dev)
            self._sumsq_ws = torch.empty(ops.backend_op("grad_sumsq_blocks")(self.params.total), dtype=torch.float64, device=dev)
        self.acc = torch.zeros(4, 8, dtype=torch.float64, device=dev)   # bce / mse / kl per pass (+ unmasked bce: --mask-loss)
        self.loss = torch.zeros(1, device=dev)
        self.partials = torch.zeros(8, device=dev)
        # the KL weight of the annealing schedule (problems.py:212-216) lives on the device: the loss assembly and the
        # latent backward read it from there, so a captured step serves every epoch without re-capture
        self.klw = torch.zeros(1, device=dev)
        self._klw_host = None
        if process_group is not None:
            # replicas must start identical whatever each rank's seeding was: rank 0's parameters and BatchNorm buffers
            import torch.distributed as dist
            dist.broadcast(self.params.flat, 0, group=process_group)
            for b in model.buffers():
                dist.broadcast(b, 0, group=process_group)
        # Exponential moving average of the parameters (None: off -- no buffer, optimizer_step is the calls it has always been).  A
        # second flat fp32 buffer that starts as the parameters (after the broadcast above, so every rank starts from rank 0's) and
        # that the Adam launch itself moves towards the parameters it writes (mmdyn_adam_step_ema: one more one-thread launch, the
        # EMA tick, and two more streams through the same pass).  Count, decay and warm-up live in four doubles on the device and
        # nothing reads the host, so the captured step keeps the average on every replay.  Every rank applies the same update to the
        # same parameter bits: the averages agree without a collective.  Fixed per engine, so the capture key does not carry it.
        self.ema_decay = None if ema_decay is None else ops.check_ema_decay(ema_decay, "ema_decay")
        self.ema_warmup = bool(ema_warmup)
        self.ema = self.ema_flat = self.ema_state = self._ema_model = None      # ema: parameter name -> view of ema_flat
        if self.ema_decay is not None:
            self.ema_flat = self.params.flat.clone()
            self.ema_state = ops.new_ema_state(self.ema_decay, self.ema_warmup, dev)
            self.ema = {k: self.ema_flat[o:o + self.params.P[k].numel()].view(self.params.P[k].shape)
                        for k, o in self.params.offsets.items()}
        self.last = {}
        self.last_rows = None            # a step with sample_weight: the unweighted per-sample tables of its batch (dict, see forward)
        self.lanes = _Lanes(dev, two_lanes)
        # every weight repack of a step (conv tap-major packs, FC permutations / transposes, fused heads) as ONE
        # kernel launch over a device-resident plan; the emulation backend packs per stack instead
        self.plan = None
        # The fused heads of the visual / tactile (/ pose) encoders as ONE grouped launch each way at the product-of-experts
        # join: equal head shapes (the unconditional models; a condition widens the image heads only)
        # and gradients laid out [G][2L][K] in the flat buffer.  Otherwise each encoder launches its own heads.
        self._head_prefixes = [p for p in HEAD_GROUP_ORDER if p != "pose_encoder" or self.use_pose]
        self._hg_grad = None if (self.conditional or not group_heads) else self.params.grouped_heads_grad(self._head_prefixes)
        self._hg_all, self._hg_views = None, None
        if self._hg_grad is not None:
            self._hg_all, self._hg_views = layers.heads_group_buffers([self.params.sub(p) for p in self._head_prefixes],
                                                                      self.params.flat, w_dtype(precision))
        if ops.B.name == "hip":
            FP = self.params
            specs = {"ev": layers.encoder_pack_specs(FP.sub("visual_encoder")),
                     "et": layers.encoder_pack_specs(FP.sub("tactile_encoder")),
                     "hv": layers.heads_pack_specs(FP.sub("visual_encoder")),
                     "ht": layers.heads_pack_specs(FP.sub("tactile_encoder")),
                     "dv": layers.decoder_pack_specs(FP.sub("visual_decoder")),
                     "dt": layers.decoder_pack_specs(FP.sub("tactile_decoder"))}
            if self.use_pose:
                specs["hp"] = layers.heads_pack_specs(FP.sub("pose_encoder"))
                # W^T of the pose MLPs' 512-wide layers (their input-gradient GEMMs' operand) ride on the late half of the plan
                specs["pe"] = layers.pose_mlp_pack_specs(FP.sub("pose_encoder"), ["fc_net.2.weight"])
                specs["pd"] = layers.pose_mlp_pack_specs(FP.sub("pose_decoder"), ["deconv_net.0.weight", "deconv_net.2.weight"])
            # what the encoder forward reads goes first (critical path); the transposed / decoder packs are launched
            # next to the encoder phase (run_late) and are ready long before the decoders start
            pre = None
            if self._hg_views is not None:     # the grouped launches' operands: the plan packs straight into their slices
                pre = {"h" + p[0]: v for p, v in zip(self._head_prefixes, self._hg_views)}
            self.plan = layers.PackPlan(specs, early=("W1p", "W2k", "W3k", "W4k", "W5k", "W6k", "Wf", "Wh", "bh"),
                                        w_dtype=w_dtype(precision), prealloc=pre, plane_twins=precision == "fp32x3")
        self._capturing = False
        self._graph = None
        self._static_mask = self._static_cond = None

    def _drop_graph(self):
        """Forget the captured step; its launches' arrival-counter slots (ops.HipBackend._ticket) become free again."""
        g, self._graph = self._graph, None
        if g is not None and len(g) > 3 and g[3]:
            torch.cuda.synchronize()            # no replay of the dropped graphs may still be using a slot
            ops.B.ticket_release(g[3])

    def close(self):
        """Drop the captured HIP graphs (and their memory pools).  Call before tearing down the process group of a
        data-parallel run: graphs that captured RCCL collectives should not outlive their communicators."""
        self._drop_graph()
        self.ctx = None
        if self.lanes.on:
            torch.cuda.synchronize()
        # the pack plan's plane twins (6 bytes per convolution weight) are registered in layers.PLANE_TWIN by strong reference:
        # a closed engine gives them back
        for ptr, pl in getattr(self.plan, "twins", None) or ():
            ent = layers.PLANE_TWIN.get(ptr)
            if ent is not None and ent[1] is pl:
                del layers.PLANE_TWIN[ptr]

    # ------------------------------------------------------------------------------------------
    def _noise(self):
        from .models.vae import NoiseSource
        if self.noise is None:
            self.noise = getattr(self.model, "noise", None) or NoiseSource(0)
        return self.noise

    def _draw(self, B, dev):
        """eps [P][B][L] and the dropout keep-masks of the visual / tactile passes.  An injected noise source is
        consumed in the reference's call order (per pass: visual mask, tactile mask, latent draw); the on-device
        Philox source draws each block with one launch."""
        n = self._noise()
        nv, nt = len(self.pass_v), len(self.pass_t)
        if hasattr(n, "_eps"):                       # InjectedNoise: keep the reference's interleaved order
            eps, mv, mt = [], [], []
            for a, b, _ in self.subsets:
                if a:
                    mv.append(n.keep_mask((B, 512), dev))
                if b:
                    mt.append(n.keep_mask((B, 512), dev))
                eps.append(n.eps((B, self.L), dev))
            return torch.stack(eps), torch.stack(mv), torch.stack(mt)
        mv = n.mask_block(nv, B, 512, dev)
        mt = n.mask_block(nt, B, 512, dev)
        eps = n.eps_block(self.P, B, self.L, dev)
        n.commit()
        return eps, mv, mt

    def _buffers(self, prefix):
        mod = getattr(self.model, prefix)
        return mod.bn_buffers()

    # ------------------------------------------------------------------------------------------
    # The step is cut into PHASES.  A phase issues kernels on whatever stream is current; "steps" phases are
    # generators yielding after every layer so that two of them can be enqueued in alternation
    # (layers.interleave).  forward()/backward() run them eagerly over the lanes; train_step_graphed() captures
    # each phase into its own HIP graph and replays the visual / tactile phases concurrently on two streams.
    # ------------------------------------------------------------------------------------------
    _MOD = {"v": ("visual_encoder", "visual_decoder", 0), "t": ("tactile_encoder", "tactile_decoder", 1)}

    def _set_kl_weight(self, kl_weight):
        if self._klw_host != float(kl_weight) and not self._capturing:
            self.klw.fill_(float(kl_weight))
            self._klw_host = float(kl_weight)

    def _check_weights(self, sample_weight, kl, B):
        """The per-sample weights in the form the kernels take (fp32 [B], contiguous, on the step's device), or None."""
        if kl not in ("batch", "sample"):
            raise ValueError("kl must be 'batch' (the reference's row: the batch-total KL) or 'sample'")
        if sample_weight is None:
            return None
        if self.pg is not None:
            raise ValueError("sample_weight with a process group is not built: data-parallel weighting is out of scope")
        if not torch.is_tensor(sample_weight) or sample_weight.numel() != B or sample_weight.dim() > 2 or \
                not sample_weight.dtype.is_floating_point:
            raise ValueError(f"sample_weight must be a floating-point tensor of B = {B} values")
        for name in ("bce_logits_rows_groups_grad", "mse_rows_groups_grad", "poe_bwd_weighted", "elbo_assemble_weighted"):
            ops.backend_op(name)         # a backend without the weighted ops: an error before anything is launched
        return sample_weight.detach().reshape(B).to(device=self.params.flat.device, dtype=torch.float32).contiguous()

    def _check_avail(self, available, target_available, B):
        """The availability tables of a mixed-modality step in the form the kernels take (:class:`_AvailTables` of uint8 [B][4] tables
        on the step's device), or None when neither is given.  Shapes and dtypes are checked, contents never looked at."""
        if isinstance(available, _AvailTables):
            return available                     # (the captured step's static tables, checked when they were made)
        if available is None and target_available is None:
            return None
        if self.pg is not None:
            raise ValueError("available / target_available with a process group is not built: data-parallel training on "
                             "mixed-modality batches is out of scope")
        from .models.functional import availability_table
        dev = self.params.flat.device
        inp = None if available is None else availability_table(available, B, dev)
        tgt = inp if target_available is None else availability_table(target_available, B, dev)
        for name in ("bce_logits_rows_groups_grad", "mse_rows_groups_grad", "poe_fwd_avail", "poe_bwd_avail_weighted", "term_weights",
                     "elbo_assemble_avail_weighted"):
            ops.backend_op(name)         # a backend without these ops: an error before anything is launched
        return _AvailTables(inp, tgt)

    def _begin(self, inputs, targets, kl_weight, train, loss_mask=None, condition=None, sample_weight=None, kl="batch", avail=None):
        sample_weight = self._check_weights(sample_weight, kl, inputs[0].shape[0])
        avail = self._check_avail(avail, None, inputs[0].shape[0])
        self._set_kl_weight(kl_weight)
        if self.conditional:
            from .models.vae import _condition
            condition = _condition(condition, True, self.categorical)
            if condition.dim() != (1 if self.categorical else 2) or condition.shape[0] != inputs[0].shape[0]:
                raise ValueError(f"condition {tuple(condition.shape)} does not match the batch of {inputs[0].shape[0]}")
            if self.categorical and self._bad_index is None:
                self._bad_index = torch.zeros(1, dtype=torch.int32, device=inputs[0].device)
        elif condition is not None:
            raise ValueError("a condition was passed to an unconditional model")
        if loss_mask is not None:
            # torch.mul(recon_i, loss_mask) of problems.py:445-447: image-shaped, so the reference fails on the (B, 7) pose term
            if self.use_pose:
                raise ValueError("loss_mask is image-shaped and cannot multiply the (B, 7) pose term (use_pose=False)")
            if loss_mask.dim() == 3:
                loss_mask = loss_mask.unsqueeze(1)
            if loss_mask.dim() != 4 or loss_mask.shape[0] != inputs[0].shape[0] or loss_mask.shape[1] not in (1, targets[0].shape[1]) \
                    or tuple(loss_mask.shape[2:]) != tuple(targets[0].shape[2:]):
                raise ValueError(f"loss_mask {tuple(loss_mask.shape)} does not broadcast over targets {tuple(targets[0].shape)}")
            loss_mask = loss_mask.to(torch.float32).contiguous()
        if not self.params.still_attached():
            raise RuntimeError("model parameters were re-allocated (e.g. .to()/.cuda() after MVAEStep was built); "
                               "construct MVAEStep after moving the model")
        v = inputs[0].contiguous()
        if self._scale_per_sample:
            # (the latent gradient is a sum over the pixels of the reconstructions: the encoder-side gradients grow with the
            #  image area, the scale shrinks with it -- 256x256 at 4 * B overflowed fp16 in the first encoder layers)
            self.loss_scale = self._scale_per_sample * v.shape[0] * (64.0 / v.shape[-1]) ** 2
        self.ctx = {"B": v.shape[0], "dev": v.device, "x": {"v": v, "t": inputs[1].contiguous()},
                    "tg": {"v": targets[0].contiguous(), "t": targets[1].contiguous()},
                    "pose": inputs[2].contiguous() if self.use_pose else None,
                    "pose_tg": targets[2].contiguous() if self.use_pose else None,
                    "kl_weight": float(kl_weight), "train": train, "pk": {}, "lmask": loss_mask, "cond": condition,
                    "rows": None,                 # score_step: fp64 [4][P][B] per-sample bce / mse / kl / unmasked-bce tables
                    # per-sample weights (fp32 [B]) of the training loss and the KL mode: the row tables are then allocated by the
                    # pre-phase, the three gradient seeds take weight vectors, the assembly is the weighted one
                    "w": sample_weight, "kl_mode": 1 if kl == "sample" else 0, "w_kl": None,
                    # a mixed-modality step (_AvailTables or None): it takes the row-table path too, with one table and one seed
                    # weight vector per TERM -- "wt" (visual, tactile, pose), written by the pre-phase's term-weight launch
                    "avail": avail, "row_path": sample_weight is not None or avail is not None,
                    "wt": {"v": sample_weight, "t": sample_weight, "p": sample_weight}}

    def _passes_of(self, m):
        return self.pass_v if m == "v" else self.pass_t

    def _dec_passes(self, m):
        """Passes the image decoder of modality ``m`` is run on (group order = pass order)."""
        return list(range(self.P)) if self.exact_running_stats else self._passes_of(m)

    def _ph_pre(self):
        """Weight repack (one launch, side lane) overlapped with the noise draws."""
        c, LN = self.ctx, self.lanes
        LN.fork()
        if self.plan is not None:
            with LN.lane(1):
                self.plan.run_early()
            c["pk"] = self.plan.packed
        c["eps"], mv, mt = self._draw(c["B"], c["dev"])
        c["mask"] = {"v": mv, "t": mt}
        LN.join()
        self.acc.zero_()
        if c["avail"] is not None:
            # bce (visual) / mse / kl / unmasked bce (visual) as below, then the tactile term's bce and unmasked bce: the two image
            # decoders do not add into one table, the assembly selects per (row, term)
            c["rows"] = torch.zeros(6, self.P, c["B"], dtype=torch.float64, device=c["dev"])
            if c["train"]:
                wt = torch.empty(3, c["B"], device=c["dev"])
                ops.B.term_weights(c["avail"].tgt, c["w"], wt, c["B"])
                c["wt"] = {"v": wt[0], "t": wt[1], "p": wt[2]}
        elif c["w"] is not None:                  # (inside the captured region: a replay starts from cleared tables)
            c["rows"] = torch.zeros(4, self.P, c["B"], dtype=torch.float64, device=c["dev"])
        if self._bad_index is not None:
            self._bad_index.zero_()
        if self._hg_grad is not None:
            # operand of the grouped heads launch: the (dropped-out) features of every pass of every encoder, group-major
            c["hg_rows"] = len(self.pass_v) * c["B"]
            c["hd_all"] = torch.empty(len(self._head_prefixes) * c["hg_rows"], 512, device=c["dev"])
            if self.plan is None:              # (emulation backend: no pack plan -- pack the heads into the group buffers here)
                for p, v in zip(self._head_prefixes, self._hg_views):
                    layers.pack_now(layers.heads_pack_specs(self.params.sub(p)), pre=v)

    def _hd_slice(self, key, gi):
        r = self.ctx["hg_rows"]
        return self.ctx[key][gi * r:(gi + 1) * r]

    def _ph_pack_late(self):
        """Decoder and backward (transposed) weight packs: on the joint stream while the lanes run the encoders."""
        if self.plan is not None:
            self.plan.run_late()

    def _ph_enc_steps(self, m):
        """Encoder trunk once per modality; per-pass dropout batched; fused heads for all passes of the modality."""
        c, FP, B = self.ctx, self.params, self.ctx["B"]
        enc = self._MOD[m][0]
        n = len(self._passes_of(m))
        h, c["e" + m] = yield from layers.encoder_trunk_forward_steps(FP.sub(enc), self._buffers(enc), c["x"][m], 1, n,
                                                                     c["pk"].get("e" + m))
        if self._hg_grad is not None:          # grouped heads: the launch follows the lanes' join (_ph_heads)
            ops.B.dropout_expand(h, c["mask"][m], self._hd_slice("hd_all", self._MOD[m][2]), n, B, 512, DROPOUT_P)
            return
        hd = torch.empty(n * B, 512, device=c["dev"])
        ops.B.dropout_expand(h, c["mask"][m], hd, n, B, 512, DROPOUT_P)
        cond = layers.repeat_condition(c["cond"], n)                           # the same condition rows for every pass
        c["o" + m], c["h" + m] = layers.heads_forward(FP.sub(enc), hd, c["pk"].get("h" + m), cond=cond)

    def _ph_pose_enc(self):
        c, FP = self.ctx, self.params
        c["op"] = None
        if self.use_pose:
            pose_rep = c["pose"].repeat(len(self.pass_p), 1)                  # same pose rows for each pass
            if self._hg_grad is not None:
                _, c["ep"] = layers.pose_encoder_trunk_forward(FP.sub("pose_encoder"), pose_rep, out=self._hd_slice("hd_all", 2))
                return
            hp, c["ep"] = layers.pose_encoder_trunk_forward(FP.sub("pose_encoder"), pose_rep)
            c["op"], c["hp"] = layers.heads_forward(FP.sub("pose_encoder"), hp, c["pk"].get("hp"))

    def _ph_heads(self):
        """Grouped heads of every encoder, one launch (joint stream, after the lanes' join)."""
        c = self.ctx
        if self._hg_grad is None:
            return
        G = len(self._head_prefixes)
        c["o_all"] = layers.heads_forward_grouped(c["hd_all"], self._hg_all, G, c["hg_rows"])
        c["ov"], c["ot"] = self._hd_slice("o_all", 0), self._hd_slice("o_all", 1)
        c["op"] = self._hd_slice("o_all", 2) if self.use_pose else None

    def _ph_heads_bwd(self):
        """Input gradients of the grouped heads (one grouped launch, joint stream): what the encoders' backward waits for."""
        c = self.ctx
        if self._hg_grad is None:
            return
        c["dhd_all"] = layers.heads_backward_grouped(c["do_all"], self._hg_all, len(self._head_prefixes), c["hg_rows"])

    def _ph_heads_wgrad(self):
        """Parameter gradients of the grouped heads: nothing on the backward chain reads them, so they run on the joint stream
        NEXT TO the lanes' encoder backward (with them in front of the fork the step measured 0.07 ms slower, same box)."""
        c = self.ctx
        if self._hg_grad is None:
            return
        layers.heads_wgrad_grouped(c["hd_all"], c["do_all"], self._hg_all, self._hg_grad[0], self._hg_grad[1],
                                   len(self._head_prefixes), c["hg_rows"])

    def _ph_poe(self):
        """Product of experts + reparametrisation + KL for every pass, one launch."""
        c, B, L, P, dev = self.ctx, self.ctx["B"], self.L, self.P, self.ctx["dev"]
        c["mu"], c["lv"], c["z"] = (torch.empty(P, B, L, device=dev) for _ in range(3))
        # the decoders' stacked inputs (torch.cat of the passes each decoder runs on: vae.py:157-163 per pass) are written by the
        # same launch: every pass's z goes to its row block of each decoder that consumes it
        lists = {"v": self._dec_passes("v"), "t": self._dec_passes("t"), "p": self.pass_p if self.use_pose else []}
        for m, pl in lists.items():
            c["zz" + m] = torch.empty(len(pl) * B, L, device=dev) if pl else None
        # fp32x3: an image decoder whose Linear layer the plane-ring kernel serves gets its stacked input already split as well
        zpl = {}
        for m in ("v", "t"):
            pl = lists[m]
            ok = (self.precision == "fp32x3" and not self.conditional and c["train"] and L % 32 == 0 and ops.B.name == "hip"
                  and layers.dense_planes_served(len(pl) * B, L, layers.FEAT))
            zpl[m] = ops.Planes(len(pl) * B, L, dev) if ok else None
            c["zzpl" + m] = zpl[m]
        passes = self._passes(c, B, None)
        for p, d in enumerate(passes):
            d["zdst"] = [c["zz" + m][pl.index(p) * B:(pl.index(p) + 1) * B] if p in pl else None for m, pl in lists.items()]
            d["zpl"] = [zpl[m].t.data_ptr() + lists[m].index(p) * B * 3 * L * 2 if (zpl.get(m) is not None and p in lists[m]) else None
                        for m in ("v", "t")]
        if c["avail"] is not None:     # the SAME input table for every pass: the pass's subset is in its null pointers, as always
            ops.B.poe_fwd_avail(passes, [c["avail"].inp] * P, c["eps"], c["mu"], c["lv"], c["z"], self.acc[2], True, P, B, L)
        else:
            ops.B.poe_fwd(passes, c["eps"], c["mu"], c["lv"], c["z"], self.acc[2], True, P, B, L)
        if c["rows"] is not None:
            ops.B.kl_rows(c["mu"], c["lv"], c["rows"][2], P, B, L)

    def _ph_dec_fwd_steps(self, m):
        """Image decoder on its live passes (groups) followed by the BCE sums (+ logit gradients when training)."""
        c, FP, B = self.ctx, self.params, self.ctx["B"]
        dec, plist, live = self._MOD[m][1], self._dec_passes(m), self._passes_of(m)
        zz = c["zz" + m]
        cond = layers.repeat_condition(c["cond"], len(plist))
        # every live pass of the modality against the same target: one loss slot per pass
        # (slot -1: exact_running_stats ran a pass whose reconstruction is discarded -- zero gradient, no loss)
        tg, mk = c["tg"][m], c["lmask"]
        slots = [p if p in live else -1 for p in plist]
        joint = self.subsets.index((1, 1, 1)) if self.use_pose else 0
        # the BCE term rides in the last decoder layer's epilogue (layers.decoder_forward_steps(loss=...)): the logits of the
        # passes nobody reads are never written; ``keep_logits`` materialises all of them (self.last["logits_*"])
        spec = dict(target=tg, slots=slots, acc=self.acc[0], grad_scale=self.loss_scale / B, want_grad=c["train"],
                    keep=None if self.keep_logits else plist.index(joint), mask=mk,
                    mask_channels=1 if mk is None else mk.shape[1], acc_u=None if mk is None else self.acc[3])
        rows = c["rows"]
        # (a mixed-modality step: the tactile term has tables of its own, and each term its own seed weights)
        kb, ku = (4, 5) if (c["avail"] is not None and m == "t") else (0, 3)
        wrec = c["wt"][m]
        if rows is not None:
            spec.update(rows=rows[kb], rows_u=None if mk is None else rows[ku], weights=wrec)
        lg, c["d" + m] = yield from layers.decoder_forward_steps(FP.sub(dec), self._buffers(dec), zz, len(plist),
                                                                 packed=c["pk"].get("d" + m), cond=cond, loss=spec if FUSED_BCE else None,
                                                                 z_planes=c.get("zzpl" + m))
        if c["d" + m]["loss_fused"]:
            c["lg" + m], c["dl" + m] = lg, c["d" + m]["dl"]
            c["lg_joint_only" + m] = not self.keep_logits
            return
        c["lg_joint_only" + m] = False
        if rows is not None and wrec is not None and c["train"]:
            dl = torch.empty_like(lg)
            ops.B.bce_logits_rows_groups_grad(lg, tg, dl, wrec, rows[kb], slots, B, tg[0].numel(), self.loss_scale / B, mask=mk,
                                              hw=tg[0, 0].numel(), mask_channels=1 if mk is None else mk.shape[1],
                                              unmasked_rows=None if mk is None else rows[ku])
            c["lg" + m], c["dl" + m] = lg, dl
            return
        if rows is not None:
            ops.B.bce_logits_rows_groups(lg, tg, rows[kb], slots, B, tg[0].numel(), mask=mk, hw=tg[0, 0].numel(),
                                         mask_channels=1 if mk is None else mk.shape[1],
                                         unmasked_rows=None if mk is None else rows[ku])
            c["lg" + m], c["dl" + m] = lg, None
            return
        dl = torch.empty_like(lg) if c["train"] else None
        if mk is None:
            ops.B.bce_logits_groups(lg, tg, dl, self.acc[0], slots, tg.numel(), self.loss_scale / B)
        else:
            ops.B.bce_logits_groups(lg, tg, dl, self.acc[0], slots, tg.numel(),
                                    self.loss_scale / B, mask=mk, chw=tg[0].numel(), hw=tg[0, 0].numel(), mask_channels=mk.shape[1],
                                    unmasked_slots=self.acc[3])
        c["lg" + m], c["dl" + m] = lg, dl

    def _ph_pose_dec_fwd(self):
        c, FP, B = self.ctx, self.params, self.ctx["B"]
        c["pr"], c["dpr"] = None, None
        if self.use_pose:
            zp = c["zzp"]
            pr, c["dp"] = layers.pose_decoder_forward(FP.sub("pose_decoder"), zp)
            dpr = torch.empty_like(pr) if c["train"] else None
            # every pose-bearing pass against the same target: one launch, one loss slot per pass
            if c["rows"] is not None and c["wt"]["p"] is not None and c["train"]:
                ops.B.mse_rows_groups_grad(pr, c["pose_tg"], dpr, c["wt"]["p"], c["rows"][1], list(self.pass_p), B, 7,
                                           self.loss_scale * self.pose_multiplier / B)
            elif c["rows"] is not None:
                ops.B.mse_rows_groups(pr, c["pose_tg"], c["rows"][1], list(self.pass_p), B, 7)
            else:
                ops.B.mse_groups(pr, c["pose_tg"], dpr, self.acc[1], list(self.pass_p), B * 7,
                                 self.loss_scale * self.pose_multiplier / B)
            c["pr"], c["dpr"] = pr, dpr

    def _ph_assemble(self):
        c = self.ctx
        if c["avail"] is not None:
            return self._assemble_avail()
        if c["rows"] is not None:
            # the per-pass sums eval_step would have produced are the sums of the rows (no second run of the scalar kernels)
            for k, used in ((0, True), (1, self.use_pose), (3, c["lmask"] is not None)):
                if used:                          # (acc was zeroed by _ph_pre: an unused table's sums stay zero)
                    torch.sum(c["rows"][k], 1, out=self.acc[k][:self.P])
        if c["w"] is not None:
            # L = (1/B) sum_b w_b row_b and its per-pass parts; the unweighted rows / partials of the batch ride along
            B, P, tab = c["B"], self.P, c["rows"]
            out, partials = torch.empty(B, device=c["dev"]), torch.empty(P, B, device=c["dev"])
            # kl="batch": the batch-total KL sits in every row, so its gradient is weighted by sum_b w_b -- written as a [B] vector
            # by the same launch (nothing synchronises with the host); kl="sample": the weights themselves
            c["w_kl"] = c["w"] if c["kl_mode"] else torch.empty(B, device=c["dev"])
            ops.B.elbo_assemble_weighted(tab[0], tab[1] if self.use_pose else None, tab[2], self.acc[2], c["w"], self.loss,
                                         self.partials, out, partials, None if c["kl_mode"] else c["w_kl"], P, B, 1.0,
                                         self.pose_multiplier, self.klw, c["kl_mode"])
            self.last_rows = {"rows": out, "partials": partials, "bce_rows": tab[0], "mse_rows": tab[1], "kl_rows": tab[2],
                              "unmasked_bce_rows": tab[3] if c["lmask"] is not None else None,
                              "kl": "sample" if c["kl_mode"] else "batch"}
            return
        ops.B.elbo_assemble(self.acc[0], self.acc[1], self.acc[2], self.loss, self.partials, self.P, c["B"],
                            1.0, self.pose_multiplier, self.klw)

    def _assemble_avail(self):
        """The loss of a mixed-modality step: a (row, term) whose target is absent is selected out of the per-term tables (and
        written back as 0), the KL counts for every row, the division stays by B; ``self.acc`` is then formed from the filtered
        tables, so the performance measures see present targets only."""
        c, B, P, tab, dev = self.ctx, self.ctx["B"], self.P, self.ctx["rows"], self.ctx["dev"]
        tgt, mk = c["avail"].tgt, c["lmask"]
        out, partials = torch.empty(B, device=dev), torch.empty(P, B, device=dev)
        present, sums = torch.empty(3, dtype=torch.float64, device=dev), torch.empty(3, P, dtype=torch.float64, device=dev)
        # the KL seed's row weights: kl="sample" the weights themselves (ones without), kl="batch" sum_b w_b in every row
        if c["kl_mode"]:
            c["w_kl"] = c["w"] if c["w"] is not None else torch.ones(B, device=dev)
        else:
            c["w_kl"] = torch.empty(B, device=dev)
        ops.B.elbo_assemble_avail_weighted(tab[0], tab[4], tab[1] if self.use_pose else None, tab[2], self.acc[2], c["w"], tgt,
                                           self.loss, self.partials, out, partials, None if c["kl_mode"] else c["w_kl"], present,
                                           sums, P, B, 1.0, self.pose_multiplier, self.klw, c["kl_mode"])
        torch.add(sums[0], sums[1], out=self.acc[0][:P])
        self.acc[1][:P].copy_(sums[2])
        unmasked = None
        if mk is not None:               # (--mask-loss: the plain sums beside the masked ones, selected the same way)
            for k, col in ((3, 0), (5, 1)):
                if tgt is not None:
                    tab[k].copy_(torch.where(tgt[:, col] != 0, tab[k], torch.zeros_like(tab[k])))
            unmasked = tab[3] + tab[5]
            torch.sum(unmasked, 1, out=self.acc[3][:P])
        self.last_rows = {"rows": out, "partials": partials, "bce_rows": tab[0] + tab[4], "mse_rows": tab[1], "kl_rows": tab[2],
                          "unmasked_bce_rows": unmasked, "kl": "sample" if c["kl_mode"] else "batch",
                          # per term (visual, tactile, pose): the tables, the number of rows that hold each target, and each
                          # term's per-pass sum over those rows
                          "bce_v_rows": tab[0], "bce_t_rows": tab[4], "present": present, "term_sums": sums,
                          "unmasked_bce_v_rows": None if mk is None else tab[3], "unmasked_bce_t_rows": None if mk is None else tab[5]}

    def _ph_dec_bwd_steps(self, m):
        c, FP = self.ctx, self.params
        dec = self._MOD[m][1]
        wq = c.setdefault("wq" + m, []) if self.defer_wgrad else None
        c["dz" + m] = yield from layers.decoder_backward_steps(FP.sub(dec), c["d" + m], c["dl" + m], FP.sub(dec, "G"), defer=wq)

    def _ph_dec_wgrad(self, m, tail=None, head=None):
        """The decoder's queued weight-gradient GEMMs (defer_wgrad), on whatever stream is current.  ``tail`` = k: only the last k
        entries of the queue (LAB, MMDYN_WGRAD_TAIL: run at the end of the lane's own encoder backward instead of behind the main
        stream's work)."""
        q = self.ctx.get("wq" + m) or []
        # (graph capture: the operands stay referenced until the step's context goes, so that no later capture into the
        #  producing lane's pool can be handed their memory while this queue's graph may still be reading it at replay)
        self.ctx.setdefault("wkeep" + m, []).extend(q)
        if head is not None:                  # the first ``head`` entries (those queued before the decoder row was cut, _capture)
            part = q[:head]
            del q[:head]
            layers.run_deferred_wgrads(part)
            return
        if tail:
            idx = os.environ.get("MMDYN_WGRAD_LANE_IDX")          # (LAB: explicit queue positions instead of the last k)
            pick = sorted({int(i) % len(q) for i in idx.split(",")}) if (idx and q) else list(range(len(q) - min(tail, len(q)), len(q)))
            part = [q[i] for i in pick]
            for i in reversed(pick):
                del q[i]
            layers.run_deferred_wgrads(part)
            return
        layers.run_deferred_wgrads(q)

    def _ph_pose_dec_bwd(self):
        c, FP = self.ctx, self.params
        c["dzp"] = None
        if self.use_pose:
            c["dzp"] = layers.pose_decoder_backward(FP.sub("pose_decoder"), c["dp"], c["dpr"], FP.sub("pose_decoder", "G"),
                                                    packed=c["pk"].get("pd"))

    def _ph_poe_bwd(self):
        """Latent gradients of every pass (summed over the decoders that consumed z) through PoE / KL."""
        c, B, L, P = self.ctx, self.ctx["B"], self.L, self.P
        blocks = [[None, None, None] for _ in range(P)]
        for g, p in enumerate(self._dec_passes("v")):
            if p in self.pass_v:
                blocks[p][0] = c["dzv"][g * B:(g + 1) * B]
        for g, p in enumerate(self._dec_passes("t")):
            if p in self.pass_t:
                blocks[p][1] = c["dzt"][g * B:(g + 1) * B]
        if self.use_pose:
            for g, p in enumerate(self.pass_p):
                blocks[p][2] = c["dzp"][g * B:(g + 1) * B]
        if self._hg_grad is not None:
            c["do_all"] = torch.empty_like(c["o_all"])
            c["dov"], c["dot"] = self._hd_slice("do_all", 0), self._hd_slice("do_all", 1)
            c["dop"] = self._hd_slice("do_all", 2) if self.use_pose else None
        else:
            c["dov"], c["dot"] = torch.empty_like(c["ov"]), torch.empty_like(c["ot"])
            c["dop"] = torch.empty_like(c["op"]) if self.use_pose else None
        if c["avail"] is not None:
            ops.B.poe_bwd_avail_weighted(self._passes(c, B, [c["dov"], c["dot"], c["dop"]], blocks), [c["avail"].inp] * P, c["eps"],
                                         c["mu"], c["lv"], None, None, None, self.loss_scale / B, c["w_kl"], True, P, B, L, self.klw)
            return
        if c["w"] is not None:
            ops.B.poe_bwd_weighted(self._passes(c, B, [c["dov"], c["dot"], c["dop"]], blocks), c["eps"], c["mu"], c["lv"], None,
                                   None, None, self.loss_scale / B, c["w_kl"], True, P, B, L, self.klw)
            return
        ops.B.poe_bwd(self._passes(c, B, [c["dov"], c["dot"], c["dop"]], blocks), c["eps"], c["mu"], c["lv"], None, None,
                      None, self.loss_scale / B, True, P, B, L, self.klw)

    def _ph_enc_bwd_steps(self, m):
        c, FP, B = self.ctx, self.params, self.ctx["B"]
        enc = self._MOD[m][0]
        if self._hg_grad is not None:
            dhd = self._hd_slice("dhd_all", self._MOD[m][2])
        else:
            dhd = layers.heads_backward(c["h" + m], c["do" + m], FP.sub(enc, "G"), fused=FP.fused_heads_grad(enc))
        dh = torch.empty(B, 512, device=c["dev"])
        # fp32x3: where the plane-ring kernel serves the FC layer's input gradient, dh is written already split as well
        dhp = None
        if (self.precision == "fp32x3" and ops.B.name == "hip" and layers.ACT_DTYPE == torch.float32
                and layers.dense_planes_served(B, 512, layers.FEAT)):
            dhp = ops.Planes(B, 512, c["dev"])
        # (the FC layer's Swish backward rides along: dh is dL/du5)
        ops.B.dropout_reduce(dhd, c["mask"][m], dh, len(self._passes_of(m)), B, 512, DROPOUT_P, u=c["e" + m]["u5"],
                             act=ops.ACT_SWISH, **({} if dhp is None else {"planes": dhp}))
        yield
        yield from layers.encoder_trunk_backward_steps(FP.sub(enc), c["e" + m], dh, FP.sub(enc, "G"), dh_is_du=True, dh_planes=dhp)

    def _ph_pose_enc_bwd(self):
        c, FP = self.ctx, self.params
        if self.use_pose:
            if self._hg_grad is not None:
                dhp = self._hd_slice("dhd_all", 2)
            else:
                dhp = layers.heads_backward(c["hp"], c["dop"], FP.sub("pose_encoder", "G"),
                                            fused=FP.fused_heads_grad("pose_encoder"))
            layers.pose_encoder_trunk_backward(FP.sub("pose_encoder"), c["ep"], dhp, FP.sub("pose_encoder", "G"),
                                               packed=c["pk"].get("pe"))

    def _publish(self):
        c, B, P = self.ctx, self.ctx["B"], self.P
        joint = self.subsets.index((1, 1, 1)) if self.use_pose else 0
        gv, gt = self._dec_passes("v").index(joint), self._dec_passes("t").index(joint)
        # (fused loss epilogue without keep_logits: the logits buffer holds the joint pass only)
        recon = [c["lgv"] if c["lg_joint_onlyv"] else c["lgv"][gv * B:(gv + 1) * B],
                 c["lgt"] if c["lg_joint_onlyt"] else c["lgt"][gt * B:(gt + 1) * B]]
        if self.use_pose:
            gp = self.pass_p.index(joint)
            recon.append(c["pr"][gp * B:(gp + 1) * B])
        self.last = {"recon_x": recon, "means": c["mu"][P - 1], "log_var": c["lv"][P - 1],
                     "logits_v": None if c["lg_joint_onlyv"] else c["lgv"], "logits_t": None if c["lg_joint_onlyt"] else c["lgt"],
                     "pose_recon": c["pr"], "masked": c["lmask"] is not None}

    def _two(self, phase):
        """Run a per-modality steps-phase for both modalities, lane 0 / lane 1, enqueued in alternation."""
        LN = self.lanes
        layers.interleave([(lambda: LN.lane(0), phase("v")), (lambda: LN.lane(1), phase("t"))])

    # ------------------------------------------------------------------------------------------
    @_with_precision
    def forward(self, inputs, targets, kl_weight, train=True, loss_mask=None, condition=None, rows=False, sample_weight=None,
                kl="batch", available=None, target_available=None):
        """Runs the forward schedule and the loss; with train=True also fills the loss gradients needed by
        :meth:`backward`.  Returns the device scalar loss (fp32).  ``loss_mask`` ([B][1 or C][H][W], models without pose):
        the reference's --mask-loss, multiplying logits and targets of every image term.  ``condition``: the condition of the
        --conditional models -- [B][condition_dim] real values (the shock force), or class indices [B] / [B,1] of any integer
        dtype for a categorical model (an index out of range: :meth:`check_condition`).

        ``sample_weight`` (fp32 [B], any finite values; None: the unweighted step, on exactly its launches): the loss becomes
        L = (1/B) sum_b w_b * row_b, with row_b the per-sample ELBO of :meth:`score_step` in the same ``kl`` mode -- ``"batch"``: the
        reference's ``(w * rows).sum() / B`` (problems.py:415-417, 451-456: the batch-total KL sits in every row and is weighted by
        sum_b w_b); ``"sample"``: each sample's own KL (with w = 1 this is the unweighted loss).  With ``train=True`` the three
        gradient seeds of :meth:`backward` (BCE, MSE, KL) are scaled per sample.  ``self.partials`` holds the weighted per-pass
        parts, ``self.last_rows`` the unweighted per-sample tables (``rows``, ``partials``, ``bce_rows``, ``mse_rows``,
        ``kl_rows``) as a by-product.  BatchNorm statistics are those of the UNWEIGHTED batch, as in the reference's autograd: a
        zero weight does not remove a sample from them.  Weights are not inspected (NaN / Inf propagate).

        ``available`` / ``target_available`` (None: every row holds everything, on exactly the launches above): a mixed-modality
        batch.  Tables in the forms ``models.functional.availability_table`` takes -- [B, 2] (visual, tactile; the pose counts as
        present) or [B, 3], any numeric dtype, non-zero = present, never inspected on the host.  ``available``: the posterior of
        row b in every subset pass is the prior times the pass's experts that the row holds (none: the prior alone).
        ``target_available`` (default: ``available``): the reconstruction term of modality m for row b counts iff the row holds
        that target; the KL counts for every row, and the loss stays divided by B:
        L = (1/B) sum_s sum_b w_b [ sum_{m in s, target present} rec_m(s, b) + kl_weight KL(s, b) ].  ``sample_weight`` composes
        (an absent term's weight is 0, by selection).  All B rows pass through every encoder and decoder and take part in the
        BatchNorm statistics, so the tensors of an absent (row, modality) must be FINITE in training (the dataset's constant image
        is); only the product of experts never loads them.  An absent target sends no gradient into its decoder, an absent
        (row, expert) gets exact-zero head-gradient rows.  ``self.last_rows`` then also holds ``bce_v_rows`` / ``bce_t_rows`` (the
        per-term tables, absent entries 0), ``present`` (fp64 [3]: rows that hold each target) and ``term_sums`` (fp64 [3][P])."""
        avail = self._check_avail(available, target_available, inputs[0].shape[0])
        self._begin(inputs, targets, kl_weight, train, loss_mask, condition, sample_weight, kl, avail)
        with layers.bad_index_into(self._bad_index):
            return self._forward_schedule(rows, train)

    def _forward_schedule(self, rows, train):
        LN = self.lanes
        if rows:
            if train or self.ctx["row_path"]:
                raise ValueError("rows=True is the evaluation schedule of score_step; a training step with per-sample rows takes "
                                 "sample_weight (its rows are in self.last_rows)")
            self.ctx["rows"] = torch.zeros(4, self.P, self.ctx["B"], dtype=torch.float64, device=self.ctx["dev"])
        self._ph_pre()
        LN.fork()
        self._ph_pack_late()
        self._two(self._ph_enc_steps)
        self._ph_pose_enc()
        LN.join()
        self._ph_heads()
        self._ph_poe()
        LN.fork()
        self._two(self._ph_dec_fwd_steps)
        self._ph_pose_dec_fwd()
        LN.join()
        self._ph_assemble()
        self._publish()
        return self.loss

    def bad_condition(self):
        """True when the most recent step of a categorical model held a class index outside [0, condition_dim): those rows ran
        with an all-zero condition block.  One 4-byte read from the device -- a synchronisation; no step makes it on its own."""
        return bool(self._bad_index is not None and int(self._bad_index.item()))

    def check_condition(self):
        """Raises ValueError where the reference asserts (vae.py:338).  Call it where the host synchronises anyway -- next to the
        read-back of the loss -- so that the step itself stays free of synchronisation."""
        if self.bad_condition():
            raise ValueError(f"categorical condition outside [0, {self.model.condition_dim}) in the last step")

    def _passes(self, c, B, dheads, dz_blocks=None):
        """Per-pass expert descriptors: row block of each modality's fused heads output."""
        L = self.L
        out = []
        for p, (a, b, cc) in enumerate(self.subsets):
            hs, ds = [None] * 3, [None] * 3
            for m, (flag, plist, key) in enumerate(((a, self.pass_v, "ov"), (b, self.pass_t, "ot"), (cc, self.pass_p, "op"))):
                if flag:
                    g = plist.index(p)
                    hs[m] = c[key][g * B:(g + 1) * B]
                    if dheads is not None:
                        ds[m] = dheads[m][g * B:(g + 1) * B]
            d = {"mu": [None if h is None else h[:, :L] for h in hs], "lv": [None if h is None else h[:, L:] for h in hs],
                 "dmu": [None if x is None else x[:, :L] for x in ds], "dlv": [None if x is None else x[:, L:] for x in ds],
                 "ld": [2 * L] * 3}
            if dz_blocks is not None:
                d["dz"] = dz_blocks[p]
            out.append(d)
        return out

    # ------------------------------------------------------------------------------------------
    @_with_precision
    def backward(self):
        """Reverse schedule; fills the flat gradient buffer.  Returns async all-reduce handles (if any)."""
        LN = self.lanes
        handles = []
        self._ph_pose_dec_bwd()
        LN.fork()
        self._two(self._ph_dec_bwd_steps)
        for i, m in enumerate("vt"):          # (eager launches: the queued weight gradients follow on their lane)
            with LN.lane(i):
                self._ph_dec_wgrad(m)
        LN.join()
        handles += self._reduce_bucket(0)
        self._ph_poe_bwd()
        self._ph_heads_bwd()
        LN.fork()
        self._two(self._ph_enc_bwd_steps)
        self._ph_heads_wgrad()
        self._ph_pose_enc_bwd()
        LN.join()
        handles += self._reduce_bucket(1)
        handles += self._reduce_bucket(2)
        self.ctx = None
        return handles

    def _reduce_bucket(self, i, last=None):
        """Async all-reduce(sum) of gradient bucket ``i`` (.. ``last``) of the flat buffer; the collective is ordered
        after everything already enqueued on the current stream and overlaps whatever is enqueued next."""
        if self.pg is None or self._capturing:
            return []
        import torch.distributed as dist
        lo = 0 if i == 0 else self.params.bucket_bounds[i - 1]
        hi = self.params.bucket_bounds[i if last is None else last]
        if self._grad16 is not None:
            ops.B.cast_f32_to_bf16(self.params.grad[lo:hi], self._grad16[lo:hi])
            h = _Bf16Bucket(dist.all_reduce(self._grad16[lo:hi], group=self.pg, async_op=True), self, lo, hi)
        else:
            h = dist.all_reduce(self.params.grad[lo:hi], group=self.pg, async_op=True)
        if self._warm_works is not None:
            self._warm_works.append(h)
        return [h]

    def optimizer_step(self, handles=(), loss_scale=None):
        """``loss_scale``: the scale the gradients in the flat buffer were produced with, when that is not the one of the
        latest ``_begin`` (a graph replay: the captured backward keeps the scale of its capture)."""
        for h in handles:
            h.wait()
        scale = self.loss_scale if loss_scale is None else loss_scale
        if self.ema_flat is not None:
            # the same steps with the average kept in the Adam pass (clip None: adam_step, else adam_step_clipped, same guard rule)
            if self.max_grad_norm is not None:
                ops.B.grad_sumsq(self.params.grad, self._sumsq_ws, self.clip)
                ops.B.grad_clip_coef(self.clip, 1.0 / (self.world * scale), self.max_grad_norm)
            ops.B.adam_step_ema(self.params.flat, self.params.grad, self.adam_m, self.adam_v, self.ema_flat, self.adam_state,
                                self.clip, self.ema_state, self.lr, self.betas[0], self.betas[1], self.eps,
                                1.0 / (self.world * scale), guarded=bool(self._scale_per_sample))
            return
        if self.max_grad_norm is not None:
            # one read of the gradient serves the norm AND the overflow guard of the fp16 modes (a non-finite norm skips the step)
            ops.B.grad_sumsq(self.params.grad, self._sumsq_ws, self.clip)
            ops.B.grad_clip_coef(self.clip, 1.0 / (self.world * scale), self.max_grad_norm)
            ops.B.adam_step_clipped(self.params.flat, self.params.grad, self.adam_m, self.adam_v, self.adam_state, self.clip,
                                    self.lr, self.betas[0], self.betas[1], self.eps, 1.0 / (self.world * scale),
                                    guarded=bool(self._scale_per_sample))
            return
        ops.B.adam_step(self.params.flat, self.params.grad, self.adam_m, self.adam_v, self.adam_state, self.lr,
                        self.betas[0], self.betas[1], self.eps, 1.0 / (self.world * scale),
                        guarded=bool(self._scale_per_sample))

    @property
    def skipped_steps(self):
        """Optimiser steps the overflow guard of the fp16 modes has skipped so far (a gradient held inf / NaN)."""
        return int(self.adam_state[4])

    @property
    def grad_norm(self):
        """``max_grad_norm`` engines: global L2 norm of the last step's averaged, unscaled gradient before clipping (None without
        ``max_grad_norm``).  Synchronises."""
        return None if self.clip is None else float(self.clip[1])

    @property
    def clipped_steps(self):
        """Optimiser steps whose gradient was scaled down to ``max_grad_norm`` so far.  Synchronises."""
        return 0 if self.clip is None else int(self.clip[3])

    # ---- the averaged weights (ema_decay) ---------------------------------------------------------------------------------------
    def _need_ema(self):
        if self.ema_flat is None:
            raise ValueError("this engine keeps no average of its parameters: build it with ema_decay")

    @property
    def ema_updates(self):
        """Updates of the average so far: the optimiser steps that were not skipped (0 without ``ema_decay``).  Synchronises."""
        return 0 if self.ema_state is None else int(self.ema_state[0])

    def ema_params(self):
        """Parameter name -> view of ``ema_flat``, named and shaped like ``model.named_parameters()``.  The views follow training."""
        self._need_ema()
        return {k: self.ema[k] for k, _ in self.model.named_parameters()}

    def ema_state_dict(self):
        """A ``state_dict`` with the model's keys: parameters from the average, buffers (the BatchNorm running estimates, which are
        averages already, and ``num_batches_tracked``) from the live model -- torch.optim.swa_utils.AveragedModel(use_buffers=False).
        The values are the live tensors, not copies."""
        self._need_ema()
        return type(self.model.state_dict())((k, self.ema.get(k, v)) for k, v in self.model.state_dict().items())

    def ema_model(self):
        """A module of the model's class in ``eval()`` mode whose parameters ARE the views of ``ema_flat`` and whose buffers ARE the
        live model's buffer tensors: it follows training without a copy, so ``MVAEInference(step.ema_model())`` serves the average
        and ``refresh()`` after further steps packs the newer one.  Built once; later calls return the same object."""
        self._need_ema()
        if self._ema_model is None:
            import copy
            twin = copy.deepcopy(self.model)
            for k, p in twin.named_parameters():
                p.requires_grad_(False)
                p.grad = None
                p.data = self.ema[k]
            live = dict(self.model.named_buffers())
            for name, mod in twin.named_modules():
                for b in list(mod._buffers):
                    if mod._buffers[b] is not None:
                        mod._buffers[b] = live[(name + "." if name else "") + b]
            self._ema_model = twin.eval()
        return self._ema_model

    @_with_precision
    def train_step(self, inputs, targets, kl_weight, loss_mask=None, condition=None, sample_weight=None, kl="batch", available=None,
                   target_available=None):
        """zero_grad -> forward -> backward -> (all-reduce) -> Adam, as problems.py:150-155.  Gradients are
        overwritten, not accumulated, so no zero_grad pass is needed.  ``sample_weight`` / ``kl`` / ``available`` /
        ``target_available``: see :meth:`forward`."""
        loss = self.forward(inputs, targets, kl_weight, train=True, loss_mask=loss_mask, condition=condition,
                            sample_weight=sample_weight, kl=kl, available=available, target_available=target_available)
        handles = self.backward()
        self.optimizer_step(handles)
        return loss

    # ------------------------------------------------------------------------------------------
    @_with_precision
    def train_step_graphed(self, inputs, targets, kl_weight, loss_mask=None, condition=None, sample_weight=None, kl="batch",
                           available=None, target_available=None):
        """Same as :meth:`train_step`, replayed from HIP graphs: the ~300 kernel launches of a step are captured
        once per batch shape (the KL weight is read from device memory).  Each phase is its OWN graph: the visual and the tactile phases are
        linear kernel chains that are launched concurrently on two streams (a single graph with parallel branches
        was measured to run its branches mostly one after the other), the joint phases run on the caller's stream.
        Each lane captures into its own memory pool, so concurrently replayed graphs never share scratch memory.
        Inputs are copied into static buffers; random draws advance through a device-side counter and Adam's step
        count lives on the device, so every replay is a real optimiser step.  With more than one rank the gradient
        all-reduce and Adam run after the graphs.  ``sample_weight`` / ``kl`` (see :meth:`forward`): the weights are one more static
        input; the capture key carries "weighted" and the KL mode, so one captured step serves every weight vector of a shape.
        ``available`` / ``target_available``: the two tables are static inputs as well; the key carries which of them were given
        (and the KL mode), never their contents -- one capture serves every mixture of a batch shape, a replay copies the tables in."""
        sample_weight = self._check_weights(sample_weight, kl, inputs[0].shape[0])
        avail = self._check_avail(available, target_available, inputs[0].shape[0])
        if self._sync is not None and not self._sync_graph_ok:
            return self.train_step(inputs, targets, kl_weight, loss_mask, condition, sample_weight, kl, avail)      # (gloo: collectives cannot be captured)
        key = tuple(tuple(x.shape) for x in inputs) + ((tuple(loss_mask.shape),) if loss_mask is not None else ())
        if sample_weight is not None:
            key += (("weighted", kl),)
        if avail is not None:
            key += (("avail", kl, avail.inp is not None, avail.tgt is not avail.inp),)
        if condition is not None:
            from .models.vae import _condition
            condition = _condition(condition, True, self.categorical)
            key += (("cond", str(condition.dtype)) + tuple(condition.shape),)
        self._set_kl_weight(kl_weight)
        if self._graph is None or self._graph[0] != key:
            self._static_in = [x.clone() for x in inputs]
            self._static_tg = [x.clone() for x in targets]
            self._static_mask = None if loss_mask is None else loss_mask.to(torch.float32).clone()
            self._static_cond = None if condition is None else condition.clone()
            self._static_w, self._static_kl = None if sample_weight is None else sample_weight.clone(), kl
            self._static_avail = None if avail is None else avail.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            if self._sync is not None:
                self._sync.pending = []                        # keep the Work handles of the warm-up's collectives
            if self.pg is not None:
                self._warm_works = []                          # (gradient buckets: _reduce_bucket)
            try:
                with torch.cuda.stream(side):                  # warm-up outside capture (allocator, lazy init)
                    self.train_step(self._static_in, self._static_tg, kl_weight, self._static_mask, self._static_cond,
                                    self._static_w, kl, self._static_avail)
                torch.cuda.current_stream().wait_stream(side)
                if self.pg is not None:
                    self._drain_before_capture(key)
            finally:
                # a warm-up step that raises must not leave later eager steps appending to the list for ever
                self._warm_works = None
                if self._sync is not None:
                    self._sync.pending = None
            self._drop_graph()           # a recapture (new batch shape): the old graphs' arrival-counter slots go back
            mark = getattr(ops.B, "ticket_mark", None)
            if mark is not None:
                mark()
            warm_rows = self.last_rows if (sample_weight is not None or avail is not None) else None
            warm_last = self.last
            try:
                captured = self._capture(kl_weight)
            except BaseException:
                # a failed capture never becomes self._graph: the arrival-counter slots its launches drew go back now
                # (nothing of the partial capture can be replayed; the sync covers the warm-up step that used other slots)
                if mark is not None:
                    torch.cuda.synchronize()
                    ops.B.ticket_release(ops.B.ticket_take())
                raise
            slots = ops.B.ticket_take() if mark is not None else []
            # the loss scale baked into the captured backward: an eval_step or an eager step on another batch size in
            # between rewrites self.loss_scale, the replayed gradients keep this one (the eager Adam of the data-parallel
            # replay divides by it)
            self._graph = (key, captured, self.loss_scale, slots)
            if warm_rows is not None:
                # last_rows now names the captured step's static outputs, which no replay has written yet: this call's rows are
                # the warm-up step's
                for k, t in self.last_rows.items():
                    if torch.is_tensor(t):
                        t.copy_(warm_rows[k])
            # ... and so does `last` (recon_x, means, log_var, the logits): this call's outputs are the warm-up step's.  Copied, like the
            # rows, so that `last` holds this step's values AND keeps naming the buffers the replays write (once per capture)
            for k, t in self.last.items():
                many = isinstance(t, (list, tuple))
                for dst, src in zip(t if many else (t,), warm_last[k] if many else (warm_last[k],)):
                    if torch.is_tensor(dst):
                        dst.copy_(src)
            return self.loss             # the warm-up above WAS this call's optimiser step
        # the batch moves into the captured step's static buffers with ONE launch (six runtime copies before round 6)
        moves = list(zip(self._static_in + self._static_tg, list(inputs) + list(targets)))
        if loss_mask is not None:
            moves.append((self._static_mask, loss_mask.reshape(self._static_mask.shape)))
        if condition is not None:
            moves.append((self._static_cond, condition))
        if sample_weight is not None:
            moves.append((self._static_w, sample_weight))
        if avail is not None:
            moves += self._static_avail.pairs(avail)
        if COPY_MANY and all(d.dtype == s_.dtype and s_.is_cuda and s_.is_contiguous() for d, s_ in moves):
            ops.B.copy_many(moves)
        else:                        # (a batch that arrives in another type / layout / on the host: the runtime's converting copy)
            for d, s_ in moves:
                if d.data_ptr() != s_.data_ptr():
                    d.copy_(s_)
        handles = self._replay(self._graph[1])
        if self.pg is not None:
            # buckets 0 and 1 were reduced under the encoder backward graphs; the conv stacks' gradients go now
            handles += self._reduce_bucket(2)
            self.optimizer_step(handles, loss_scale=self._graph[2])
        return self.loss

    WATCHDOG_SWEEP_S = 0.1       # ProcessGroupNCCL's watchdog thread looks at its list of un-retired Work objects every 100 ms
    DRAIN_TIMEOUT_S = 60.0

    def _drain_before_capture(self, key):
        """Everything a captured step with RCCL collectives relies on, made explicit before the capture starts.

        (1) Every rank must be about to capture the SAME step (a capture on one rank only would leave the lane
        communicators waiting for collectives nobody issues): the capture keys are compared across ranks, a mismatch is an
        error on every rank instead of a hang.  (2) The warm-up's collectives must be finished: their Work handles (gradient
        buckets: kept by _reduce_bucket; SyncBN statistics: layers.SyncBN.pending) are polled with ``is_completed()`` until
        every one answers True (bounded by DRAIN_TIMEOUT_S: a Work that never completes is an error, not a hang), the device
        is synchronised, and one barrier per communicator proves that every rank got that far.  (3) The process group's
        watchdog THREAD polls the events of Work objects it has not retired yet; a poll that lands while a communicator's
        stream is capturing fails ("operation not permitted on an event last recorded in a capturing stream") and aborts the
        process.  Retirement itself cannot be observed from Python -- the ProcessGroupNCCL / Work bindings of torch 2.10 expose
        ``is_completed()``, which answers for the GPU side of a Work, and nothing about the watchdog's list -- but it follows
        from (2): every Work is complete on every rank, so the watchdog's NEXT sweep retires them all, and a sweep starts
        every WATCHDOG_SWEEP_S (the documented 100 ms; TORCH_NCCL_* settings do not change it).  2.5 sweep intervals are
        waited after the last barrier: one would do by the argument above, but the argument rests on the watchdog's timing and
        on host scheduling, no multi-rank RCCL run has measured it, and the wait is paid once per capture.
        The capture itself runs with capture_error_mode="thread_local", so API calls of other threads cannot invalidate it."""
        import time
        import torch.distributed as dist
        keys = [None] * self.world
        dist.all_gather_object(keys, repr(key), group=self.pg)
        if any(k != keys[0] for k in keys):
            raise RuntimeError(f"mmdyn_hip: ranks are about to capture different steps {keys}: every rank must see the same "
                               "batch shapes (shard evenly, drop the last partial batch)")
        groups = [self.pg]
        works = list(self._warm_works or [])
        self._warm_works = None
        if self._sync is not None:
            works += list(self._sync.pending or [])
            self._sync.pending = None
            groups += list(self._sync.lane_groups or [])
        deadline = time.monotonic() + self.DRAIN_TIMEOUT_S
        while not all(w.is_completed() for w in works):
            if time.monotonic() > deadline:
                raise RuntimeError("mmdyn_hip: a collective of the warm-up step did not complete before the graph capture")
            time.sleep(0.001)
        torch.cuda.synchronize()
        for g in groups:
            dist.barrier(group=g)
        torch.cuda.synchronize()
        time.sleep(2.5 * self.WATCHDOG_SWEEP_S)

    def _capture(self, kl_weight):
        LN = self.lanes
        run = layers.run
        # (LAB, MMDYN_DEC_SPLIT=k: the decoder row is cut after k steps of the backward; the weight gradients queued by then run on the
        #  main stream next to the rest of the decoders' backward instead of after the encoder backward -- measured WORSE, same box,
        #  alternating: k = 2: 4.97 / 4.95 / 4.96 ms, k = 3: 5.01 / 4.99 / 5.01 against 4.86 / 4.83 / 4.85 (run_ab_dec_split.sh))
        dsplit = int(os.environ.get("MMDYN_DEC_SPLIT", "0")) if (self.defer_wgrad and self.pg is None) else 0
        dgens = {}

        def dec_a(m):
            run(self._ph_dec_fwd_steps(m))
            dgens[m] = self._ph_dec_bwd_steps(m)
            for _ in range(dsplit):
                next(dgens[m])
            self.ctx["wq_n" + m] = len(self.ctx.get("wq" + m) or [])

        def dec_b(m):
            for _ in dgens.pop(m):
                pass

        stages = [
            [("main", lambda: self._ph_pre())],
            [("l0", lambda: run(self._ph_enc_steps("v"))), ("l1", lambda: run(self._ph_enc_steps("t"))),
             ("main", lambda: (self._ph_pack_late(), self._ph_pose_enc()))],
            [("main", lambda: (self._ph_heads(), self._ph_poe()))],
            [("l0", lambda: (run(self._ph_dec_fwd_steps("v")), run(self._ph_dec_bwd_steps("v")))),
             ("l1", lambda: (run(self._ph_dec_fwd_steps("t")), run(self._ph_dec_bwd_steps("t")))),
             ("main", lambda: (self._ph_pose_dec_fwd(), self._ph_pose_dec_bwd()))],
            [("main", lambda: (self._ph_assemble(), self._ph_poe_bwd(), self._ph_heads_bwd()))],
        ]
        if dsplit:
            stages[3] = [("l0", lambda: dec_a("v")), ("l1", lambda: dec_a("t")),
                         ("main", lambda: (self._ph_pose_dec_fwd(), self._ph_pose_dec_bwd()))]
            stages.insert(4, [("l0", lambda: dec_b("v")), ("l1", lambda: dec_b("t")),
                              ("main", lambda: (self._ph_dec_wgrad("v", head=self.ctx["wq_n" + "v"]),
                                                self._ph_dec_wgrad("t", head=self.ctx["wq_n" + "t"])))])
        # deferred decoder weight gradients: two more graphs of the encoder-backward row, captured on streams of their own and replayed
        # where _replay puts them.  Forking them one phase earlier, next to the serial latent backward, measured no better: 6.69 vs 6.68 ms.
        wq = [("w0", lambda: self._ph_dec_wgrad("v")), ("w1", lambda: self._ph_dec_wgrad("t"))] if self.defer_wgrad else []
        if self.pg is None:
            # the last entry of each decoder's deferred queue -- the FC layer's weight gradient, a launch that fills a fraction of the
            # chip -- runs at the end of the lane's own encoder backward, the rest behind the main stream's work (_replay): +0.7-1.6 %
            # on two boxes against the whole queue on the main stream (MMDYN_WGRAD_TAIL=0; 2: equal to 0; other single entries: equal
            # or worse -- tests/microbench/run_ab_wgrad_tail.sh, run_ab_wgrad_lane_idx.sh, profiles/r5/step_ab_wgrad_fork.txt)
            ktail = int(os.environ.get("MMDYN_WGRAD_TAIL", "1")) if self.defer_wgrad else 0
            # (LAB, MMDYN_POSE_BWD_LANE=0|1: the pose encoder's backward at the end of that lane's graph instead of on the main stream --
            #  measured worse, same box, alternating: 4.69 / 4.68 / 4.70 ms against 4.64 / 4.65 / 4.65: run_ab_pose_bwd_lane.sh)
            pl = os.environ.get("MMDYN_POSE_BWD_LANE", "") if self.defer_wgrad else ""
            stages.append([("l0", lambda: (run(self._ph_enc_bwd_steps("v")), ktail and self._ph_dec_wgrad("v", ktail),
                                           pl == "0" and self._ph_pose_enc_bwd())),
                           ("l1", lambda: (run(self._ph_enc_bwd_steps("t")), ktail and self._ph_dec_wgrad("t", ktail),
                                           pl == "1" and self._ph_pose_enc_bwd())),
                           ("main", lambda: (self._ph_heads_wgrad(), pl not in ("0", "1") and self._ph_pose_enc_bwd()))] + wq)
            stages.append([("main", lambda: self.optimizer_step(()))])
        else:
            # data parallel: the encoder backward is cut after the heads + FC layer (gradient bucket 1: 31 MB of the 37 MB
            # still to be reduced), so that bucket's all-reduce runs under the conv stacks' backward instead of after it
            gens = {}

            def head(m):
                gens[m] = self._ph_enc_bwd_steps(m)
                next(gens[m])                  # heads + dropout
                next(gens[m])                  # FC layer: weight / bias gradients and the input gradient

            def tail(m):
                for _ in gens.pop(m):
                    pass

            stages.append([("l0", lambda: head("v")), ("l1", lambda: head("t")),
                           ("main", lambda: (self._ph_heads_wgrad(), self._ph_pose_enc_bwd()))] + wq)
            stages.append([("l0", lambda: tail("v")), ("l1", lambda: tail("t"))])
        if getattr(self, "_wstreams", None) is None:
            # (the capture streams of the two queues, and their replay streams with MMDYN_WGRAD_FORK=enc|dec; ONE stream for both
            #  queues measured the same step as two, 5.28-5.30 against 5.25-5.29 ms; GPU_MAX_HW_QUEUES other than the default 4 cost
            #  4-25 %: profiles/r5/stage_timeline_and_streams.txt)
            wprio = int(os.environ.get("MMDYN_WGRAD_PRIO", "0"))
            self._wstreams = [torch.cuda.Stream(priority=wprio), torch.cuda.Stream(priority=wprio)]
        cap_stream = {"main": torch.cuda.Stream(), "l0": LN.side[0], "l1": LN.side[1], "w0": self._wstreams[0], "w1": self._wstreams[1]}
        pools = {k: torch.cuda.graph_pool_handle() for k in cap_stream}
        self._capturing = True
        lanes_on, LN.on = LN.on, False            # inside a lane graph everything stays on the capture stream ...
        captured = []
        bad_scope = layers.bad_index_into(self._bad_index)
        bad_scope.__enter__()
        try:
            self._begin(self._static_in, self._static_tg, kl_weight, True, self._static_mask, self._static_cond,
                        getattr(self, "_static_w", None), getattr(self, "_static_kl", "batch"), getattr(self, "_static_avail", None))
            for stage in stages:
                row = []
                for lane, fn in stage:
                    g = torch.cuda.CUDAGraph()
                    LN.on = lanes_on and lane == "main" and fn is stages[0][0][1]   # ... except the pre-phase fork
                    layers.CUR_LANE = {"l0": 0, "l1": 1}.get(lane)                  # (SyncBN: the lane's communicator)
                    # (thread_local: API calls of OTHER threads -- RCCL's watchdog -- must not invalidate the capture)
                    with torch.cuda.graph(g, pool=pools[lane], stream=cap_stream[lane], capture_error_mode="thread_local"):
                        fn()
                    row.append((lane, g))
                captured.append(row)
            self._publish()
        finally:
            self._capturing = False
            LN.on = lanes_on
            layers.CUR_LANE = None
            self.ctx = None
            bad_scope.__exit__(None, None, None)
        return captured

    DEC_STAGE = 3          # index of the decoder forward+backward stage in _capture's list

    def _replay(self, captured):
        LN = self.lanes
        main = torch.cuda.current_stream()
        side = {"l0": LN.side[0], "l1": LN.side[1]}
        if self.defer_wgrad:
            side.update({"w0": self._wstreams[0], "w1": self._wstreams[1]})
        handles, loose = [], []
        # (LAB, MMDYN_WGRAD_FORK=dec: each decoder's deferred weight gradients forked behind ITS OWN backward instead of next to
        #  the encoder backward -- measured WORSE, same box, alternating: 5.33 / 5.25 / 5.28 ms against 5.14 / 5.12 / 5.10 ms
        #  (tests/microbench/run_ab_wgrad_fork.sh): the full-chip weight-gradient kernels slow the other decoder's dependent chain by
        #  more than they fill of its gaps)
        fork = os.environ.get("MMDYN_WGRAD_FORK", "main")
        early = self.defer_wgrad and fork == "dec"
        # Default ("main"): the two deferred queues are replayed on the MAIN stream behind its own (short) work of the encoder-backward
        # row -- three streams in all.  Two more streams for them ("enc", rounds 3-4) measured 1.3 % slower on the same box, alternating:
        # 4.98 / 5.03 / 5.00 ms against 4.95 / 4.92 / 4.94 (profiles/r5/step_ab_wgrad_fork.txt); the step's five streams then shared four
        # hardware queues, and every other queue count or stream priority measured 4-40 % worse (stage_timeline_and_streams.txt).
        on_main = self.defer_wgrad and fork == "main"
        for ri, row in enumerate(captured):
            if ri == self.DEC_STAGE + 1 and not self.defer_wgrad:
                handles += self._reduce_bucket(0)          # decoders done: reduce them under the encoder backward
            if ri == self.DEC_STAGE + 3 and self.pg is not None:
                if self.defer_wgrad:                       # (the decoders' bucket waits for their deferred weight gradients)
                    for lane in loose:
                        main.wait_event(side[lane].record_event())
                    loose = []
                    handles += self._reduce_bucket(0, last=1)
                else:
                    handles += self._reduce_bucket(1)      # heads / pose encoder / encoder FC: under the conv stacks' backward
            if ri == len(captured) - 1:                    # the last row (optimiser, or the data-parallel tail) needs every gradient
                for lane in loose:
                    main.wait_event(side[lane].record_event())
                loose = []
            if len(row) == 1:
                row[0][1].replay()
                continue
            ev = main.record_event()
            for lane, g in row:
                if lane.startswith("w") and (early or on_main):
                    continue                               # launched behind its decoder lane, two rows up / on the main stream below
                if lane != "main":
                    side[lane].wait_event(ev)
                    with torch.cuda.stream(side[lane]):
                        g.replay()
                if ri == self.DEC_STAGE and early and lane in ("l0", "l1"):
                    # (LAB: this decoder's deferred weight gradients start as soon as ITS backward is done)
                    wl = "w" + lane[1]
                    wg = dict(captured[self.DEC_STAGE + 2]).get(wl)
                    if wg is not None:
                        side[wl].wait_event(side[lane].record_event())
                        with torch.cuda.stream(side[wl]):
                            wg.replay()
            wfirst = on_main and os.environ.get("MMDYN_WGRAD_FIRST") == "1"     # (LAB: the deferred queues in FRONT of the main stream's own work)
            if wfirst:
                for lane, g in row:
                    if lane.startswith("w"):
                        g.replay()
            for lane, g in row:
                if lane == "main":
                    g.replay()
            if on_main and not wfirst:
                for lane, g in row:
                    if lane.startswith("w"):
                        g.replay()
            for lane, g in row:
                if lane.startswith("w") and not on_main:
                    loose.append(lane)                     # joined in front of the optimiser, not at the end of this row
                elif lane != "main":
                    main.wait_event(side[lane].record_event())
        for lane in loose:
            main.wait_event(side[lane].record_event())
        return handles

    @torch.no_grad()
    @_with_precision
    def eval_step(self, inputs, targets, kl_weight, loss_mask=None, condition=None, sample_weight=None, kl="batch", available=None,
                  target_available=None):
        """``sample_weight`` / ``kl`` / ``available`` / ``target_available``: the loss of :meth:`forward` without gradients (rows in
        ``self.last_rows``)."""
        loss = self.forward(inputs, targets, kl_weight, train=False, loss_mask=loss_mask, condition=condition,
                            sample_weight=sample_weight, kl=kl, available=available, target_available=target_available)
        self.ctx = None
        return loss

    @torch.no_grad()
    @_with_precision
    def score_step(self, inputs, targets, kl_weight, loss_mask=None, condition=None, kl="batch"):
        """Per-sample ELBO of one batch: the schedule of :meth:`eval_step` (same BatchNorm mode, subset passes and lanes) ending in
        the row kernels -- the fused last decoder layer adds each block's BCE sum to its SAMPLE's entry, so no logits beyond the
        published joint reconstruction are written.  Returns a dict of device tensors:

          ``rows`` fp32 [B]: sum over the subset passes of bce + pose_multiplier * mse + kl_weight * KL, nothing divided by B.
            ``kl="batch"``: KL is the total over the batch, in every row -- what the reference's ``reduce=False`` returns
            (problems.py:429, 456); ``kl="sample"``: each sample's own KL, the quantity to rank samples by.
          ``partials`` fp32 [P][B] the same per pass; ``bce_rows`` / ``mse_rows`` / ``kl_rows`` fp64 [P][B];
          ``loss`` (fp32 scalar) and ``loss_partials`` ([P]): what ``eval_step`` returns / leaves in ``self.partials`` on the same
          inputs and noise, from the sums of the rows.  ``self.last`` / ``self.acc`` are filled as by ``eval_step``.
        Forward only."""
        if kl not in ("batch", "sample"):
            raise ValueError("kl must be 'batch' (the reference's row: the batch-total KL) or 'sample'")
        loss = self.forward(inputs, targets, kl_weight, train=False, loss_mask=loss_mask, condition=condition, rows=True)
        c, P = self.ctx, self.P
        B, tab = c["B"], c["rows"]
        out = torch.empty(B, device=c["dev"])
        partials = torch.empty(P, B, device=c["dev"])
        ops.B.elbo_assemble_rows(tab[0], tab[1] if self.use_pose else None, tab[2], self.acc[2], out, partials, P, B, 1.0,
                                 self.pose_multiplier, self.klw, 1 if kl == "sample" else 0)
        self.ctx = None
        return {"rows": out, "partials": partials, "bce_rows": tab[0], "mse_rows": tab[1], "kl_rows": tab[2],
                "unmasked_bce_rows": tab[3] if self.last["masked"] else None, "loss": loss.clone(),
                "loss_partials": self.partials[:P].clone(), "kl": kl}


class MVAEInference:
    """Forward-only serving path for a trained :class:`mmdyn_hip.models.MVAE` in ``eval()`` mode
    (MVAE.forward / MVAE.inference of the reference, vae.py:126-176, with running-estimate BatchNorm and no
    dropout -- what ``model.eval()`` gives).

    What a deployment needs and the training step does not: the weights never change, so they are packed into GEMM
    operand form ONCE (``refresh()`` after loading new weights); the visual and the tactile halves run on two HIP
    streams; and the whole forward for a given (batch shape, modality subset) is captured into a HIP graph on first
    use and replayed afterwards, so a request costs one graph launch.  Latent draws come from the device-side Philox
    stream, so replays draw fresh noise.

    Conditional models (--conditional, real-valued or categorical) are served too: ``forward`` / ``score`` take ``condition=``,
    ``inference`` takes ``c``.  The condition is joined to the 512 features in front of each image encoder's heads and to the
    latent in front of each image decoder by one mmdyn_concat_condition launch per consumer (four for a joint request); the
    packed head / up-sampling weights carry the condition columns, zero-padded to the GEMM's K-step.  A categorical model takes
    class indices; its one-hot rows are written by the join kernel.  :meth:`bad_condition` reports an index out of range.
    :meth:`plan` asks the inverse question: N candidate conditions per row are scored against a goal state and the best one is
    picked on the device, in one graph whose launch count does not grow with N (up to 8 candidates); :meth:`plan_rollout` asks it
    over a horizon: N candidate condition sequences are rolled out T steps, and the best one comes back with its trajectory;
    :meth:`plan_refine` makes and refines those sequences itself: the cross-entropy method, I iterations of draw / roll out / refit in
    one graph (real-valued conditions)."""

    def __init__(self, model, precision="fp32x3", use_graph=True, seed=0):
        from .models.vae import NoiseSource
        if precision not in PRECISIONS:
            raise ValueError("precision must be 'fp32x3' (default), 'fp32', 'bf16' / 'fp16' (matrix-core operands) or 'bf16s' / 'fp16s' (+ 16-bit "
                             "activation storage)")
        self.model, self.precision, self.use_graph = model, precision, use_graph
        # --conditional (vae.py:231-237, 286-291): the condition joins the 512 features in front of the image encoders' heads and
        # the latent in front of the image decoders' first layer; the pose MLPs are built unconditional (vae.py:117-123)
        self.conditional = bool(getattr(model, "conditional", False))
        self.categorical = self.conditional and bool(getattr(model, "categorical_conditions", False))
        self.condition_dim = int(model.condition_dim or 0) if self.conditional else 0
        self._bad = None                       # int32 [1]: bit 0 = the last request held a class index outside [0, condition_dim)
        self.use_pose = bool(model._use_pose)
        self.L = model.latent_size
        self.dev = next(model.parameters()).device
        self.lanes = _Lanes(self.dev, True)
        self.noise = NoiseSource(seed)
        self._sync = None
        self._graphs = {}
        self._zeros = {}                       # batch size -> the all-zero eps of complete(sample=False)
        self._w_dtype = w_dtype(precision)     # packed GEMM operands
        self.refresh()

    def _P(self, name, keys):
        sd = dict(getattr(self.model, name).named_parameters())
        return {k: sd[k].detach() for k in keys}

    def refresh(self):
        """(Re)pack the weights -- call after ``load_state_dict``.  Captured graphs stay valid (the packed buffers and
        the parameter storage do not move)."""
        m = self.model
        self.P = {"ve": self._P("visual_encoder", m.visual_encoder.param_keys() + layers.HEAD_KEYS),
                  "te": self._P("tactile_encoder", m.tactile_encoder.param_keys() + layers.HEAD_KEYS),
                  "vd": self._P("visual_decoder", m.visual_decoder.param_keys()),
                  "td": self._P("tactile_decoder", m.tactile_decoder.param_keys())}
        self.buf = {"ve": m.visual_encoder.bn_buffers(), "te": m.tactile_encoder.bn_buffers(),
                    "vd": m.visual_decoder.bn_buffers(), "td": m.tactile_decoder.bn_buffers()}
        if ops.B.name == "hip":
            # the running estimates do not change between requests: their mean / rstd once, not one launch per layer and request
            # (written into the tensors of the previous refresh, which captured graphs read)
            prev = getattr(self, "_eval_buf", None) or {}
            self.buf = self._eval_buf = {k: layers.precompute_eval_stats(v, prev.get(k)) for k, v in self.buf.items()}
        if self.use_pose:
            self.P["pe"] = self._P("pose_encoder", layers.POSE_ENC_KEYS + layers.HEAD_KEYS)
            self.P["pd"] = self._P("pose_decoder", layers.POSE_DEC_KEYS)
        specs = {"ve": layers.encoder_pack_specs(self.P["ve"]), "te": layers.encoder_pack_specs(self.P["te"]),
                 "vh": layers.heads_pack_specs(self.P["ve"]), "th": layers.heads_pack_specs(self.P["te"]),
                 "vd": layers.decoder_pack_specs(self.P["vd"]), "td": layers.decoder_pack_specs(self.P["td"])}
        if self.use_pose:
            specs["ph"] = layers.heads_pack_specs(self.P["pe"])
        if getattr(self, "pk", None) is None:
            if ops.B.name == "hip":
                # (fp32x3: the conv-weight packs also as plane twins -- the weights are split ONCE here, not by a launch per layer and request)
                self._plan = layers.PackPlan(specs, w_dtype=self._w_dtype, plane_twins=self.precision == "fp32x3")
                self.pk = self._plan.packed
            else:
                self._plan, self._specs = None, specs
        if self._plan is not None:
            self._plan.run()
        else:
            prev_w, layers.W_DTYPE = layers.W_DTYPE, self._w_dtype
            try:
                self.pk = {k: layers.pack_now(v) for k, v in specs.items()}
            finally:
                layers.W_DTYPE = prev_w

    def close(self):
        """Drop the captured graphs and give back the pack plan's plane twins (registered in layers.PLANE_TWIN by strong reference)."""
        self._graphs = {}
        for ptr, pl in getattr(self._plan, "twins", None) or ():
            ent = layers.PLANE_TWIN.get(ptr)
            if ent is not None and ent[1] is pl:
                del layers.PLANE_TWIN[ptr]

    # ---- the forward itself (eager; captured by _graphed) -------------------------------------------------
    def _condition(self, condition, B):
        """The request's condition in the form the join kernel takes (fp32 [B, condition_dim], or int64 class indices [B] for a
        categorical model), on the engine's device; ValueError when it is missing, surplus or of the wrong shape."""
        if not self.conditional:
            if condition is not None:
                raise ValueError("a condition was passed to an unconditional model")
            return None
        from .models.vae import _condition
        cond = _condition(condition, True, self.categorical).to(self.dev)
        want = (B,) if self.categorical else (B, self.condition_dim)
        if tuple(cond.shape) != want:
            raise ValueError(f"condition {tuple(cond.shape)} does not match the batch of {B} (condition_dim = {self.condition_dim})")
        return cond

    def _cond_key(self, cond):
        return None if cond is None else ("index" if self.categorical else "real",) + tuple(cond.shape)

    def _index_scope(self):
        """Installs the engine's bad-index word for the join launches of one request and clears it first -- inside the captured
        region, so every replay starts from a clear word."""
        if self.categorical:
            if self._bad is None:
                self._bad = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self._bad.zero_()
        return layers.bad_index_into(self._bad)

    def bad_condition(self):
        """True when the most recent request of a categorical model held a class index outside [0, condition_dim): such a row
        was served with an all-zero condition block (the reference asserts, vae.py:338).  One 4-byte read from the device: a
        synchronisation, which :meth:`forward` / :meth:`score` / :meth:`inference` do not make on their own."""
        return bool(self._bad is not None and int(self._bad.item()))

    def _trunk(self, key, x):
        """The image encoder's trunk: x -> the 512 features in front of its heads."""
        return layers.run(layers.encoder_trunk_forward_steps(self.P[key], self.buf[key], x, packed=self.pk[key], training=False))[0]

    def _image_heads(self, key, h, cond=None, x_rows=None):
        """The image encoder's fused heads on the trunk's features (joined to the condition in front of them)."""
        return layers.heads_forward(self.P[key], h, self.pk[key[0] + "h"], cond=cond, x_rows=x_rows)[0]

    def _encode(self, key, x, cond=None, x_rows=None):
        return self._image_heads(key, self._trunk(key, x), cond, x_rows)

    def _trunks(self, visual, tactile, pose):
        """The part of :meth:`_heads` that does not see the condition, for a request that runs the heads more than once: [visual
        features | None, tactile features | None, pose heads [B][2L] | None]."""
        LN = self.lanes
        out = [None, None, None]
        LN.fork()
        if visual is not None:
            with LN.lane(0):
                out[0] = self._trunk("ve", visual)
        if tactile is not None:
            with LN.lane(1):
                out[1] = self._trunk("te", tactile)
        if pose is not None and self.use_pose:
            hp, _ = layers.pose_encoder_trunk_forward(self.P["pe"], pose)
            out[2] = layers.heads_forward(self.P["pe"], hp, self.pk["ph"])[0]
        LN.join()
        return out

    def _heads_of(self, trunks, cond, x_rows=None):
        """The image heads on stored trunk outputs (:meth:`_trunks`): the heads of :meth:`_heads`, launch for launch from the
        join on; the pose entry is handed through."""
        LN = self.lanes
        heads = [None, None, trunks[2]]
        LN.fork()
        if trunks[0] is not None:
            with LN.lane(0):
                heads[0] = self._image_heads("ve", trunks[0], cond, x_rows)
        if trunks[1] is not None:
            with LN.lane(1):
                heads[1] = self._image_heads("te", trunks[1], cond, x_rows)
        LN.join()
        return heads

    @staticmethod
    def _rows_of(visual, tactile, pose, avail):
        """(B, device) of a request: from the first modality given, or from the table of a request of prior-only rows."""
        ref = visual if visual is not None else (tactile if tactile is not None else (pose if pose is not None else avail))
        return ref.shape[0], ref.device

    def _forward(self, visual, tactile, pose, cond=None, avail=None, sample=True):
        with self._index_scope():
            B, dev = self._rows_of(visual, tactile, pose, avail)
            heads = self._heads(visual, tactile, pose, cond)
            mu, lv, z = self._poe(heads, avail, self._draw_latent(B) if sample else self._zero_latent(B), B, dev)
            return self._decode(z, cond) + (mu, lv)

    def _heads(self, visual, tactile, pose, cond, x_rows=None):
        """The fused (means | log_var) head outputs [B][2L] of the modalities given, None for the others.  ``x_rows`` = B with
        ``cond`` holding N * B candidate rows: the trunks run on the B rows, the image heads on the N * B rows [h[r % B] | cond[r]]
        (the pose heads take no condition and stay [B][2L])."""
        LN = self.lanes
        heads = [None, None, None]
        LN.fork()
        if visual is not None:
            with LN.lane(0):
                heads[0] = self._encode("ve", visual, cond, x_rows)
        if tactile is not None:
            with LN.lane(1):
                heads[1] = self._encode("te", tactile, cond, x_rows)
        if pose is not None and self.use_pose:
            hp, _ = layers.pose_encoder_trunk_forward(self.P["pe"], pose)
            heads[2] = layers.heads_forward(self.P["pe"], hp, self.pk["ph"])[0]
        LN.join()
        return heads

    def _poe(self, heads, avail, eps, B, device, out=None):
        """The product-of-experts launch on the heads: (mu, lv, z), each [B][L]; ``eps`` None: the posterior alone, z is not
        written and comes back as None.  ``out``: the (mu, lv) tensors to write instead of new ones."""
        L = self.L
        mu, lv = out if out is not None else (torch.empty(B, L, device=device) for _ in range(2))
        z = None if eps is None else torch.empty(B, L, device=device)
        p = {"mu": [None if h is None else h[:, :L] for h in heads], "lv": [None if h is None else h[:, L:] for h in heads],
             "dmu": [None] * 3, "dlv": [None] * 3, "ld": [2 * L] * 3}
        if avail is None:
            ops.B.poe_fwd([p], eps, mu, lv, z, None, True, 1, B, L)
        else:       # a mixed request: the same single launch, the experts of each row chosen by the row's word of the table
            ops.B.poe_fwd_avail([p], [avail], eps, mu, lv, z, None, True, 1, B, L)
        return mu, lv, z

    def _zero_latent(self, B):
        """eps = 0: z is the posterior mean.  Allocated and cleared once per batch size, outside any captured region."""
        z = self._zeros.get(B)
        if z is None:
            z = self._zeros[B] = torch.zeros(B, self.L, device=self.dev)
        return z

    def _decode(self, z, cond=None):
        LN = self.lanes
        LN.fork()
        with LN.lane(0):
            v, _ = layers.run(layers.decoder_forward_steps(self.P["vd"], self.buf["vd"], z, packed=self.pk["vd"], cond=cond,
                                                           training=False))
        with LN.lane(1):
            t, _ = layers.run(layers.decoder_forward_steps(self.P["td"], self.buf["td"], z, packed=self.pk["td"], cond=cond,
                                                           training=False))
        pr = layers.pose_decoder_forward(self.P["pd"], z)[0] if self.use_pose else None
        LN.join()
        return v, t, pr

    def _sample(self, n, cond=None):
        with self._index_scope():
            return self._decode(self._draw_latent(n), cond)[:2]

    def _draw_latent(self, n):
        """[n, L] standard-normal draw; the commit moves the stream position into the device counter, inside the
        captured region, so that every graph replay draws fresh numbers."""
        z = self.noise.eps((n, self.L), self.dev)
        self.noise.commit()
        return z

    # ---- graph capture / replay ---------------------------------------------------------------------------
    def _run(self, key, fn, new_inputs):
        prev_act, prev_w = layers.ACT_DTYPE, layers.W_DTYPE
        prev = _select_precision(self.precision)
        layers.ACT_DTYPE = act_dtype(self.precision)
        layers.W_DTYPE = self._w_dtype
        try:
            if not (self.use_graph and self.dev.type == "cuda"):
                return fn(*new_inputs)
            ent = self._graphs.get(key)
            if ent is None:
                static = [None if x is None else x.clone() for x in new_inputs]
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):                   # warm-up outside capture
                    fn(*static)
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = fn(*static)
                ent = self._graphs[key] = (g, static, out)      # (capture records, it does not execute: replay below)
            g, static, out = ent
            moves = [(dst, src) for dst, src in zip(static, new_inputs) if dst is not None and dst.data_ptr() != src.data_ptr()]
            if COPY_MANY and len(moves) > 1 and ops.B.name == "hip" and all(d.dtype == s_.dtype and s_.is_cuda for d, s_ in moves):
                ops.B.copy_many(moves)                          # the request's inputs into the graph's static buffers: one launch
            else:
                for dst, src in moves:
                    dst.copy_(src)
            g.replay()
            return out
        finally:
            _restore_precision(prev)
            layers.ACT_DTYPE = prev_act
            layers.W_DTYPE = prev_w

    def _availability(self, available, B):
        """The request's availability as the kernels' uint8 [B][4] table on the engine's device (None stays None): a few
        element-wise torch ops before the captured region; the table's contents are not looked at."""
        if available is None:
            return None
        from .models.functional import availability_table
        return availability_table(available, B, self.dev)

    def _request(self, who, x, pose, available, cast=False):
        """The prologue of every request: ``x = [visual | None, tactile | None]`` and ``pose`` -> (three contiguous tensors / None,
        the pose dropped for a model without one; B).  ``cast``: to fp32 as well, for the requests whose inputs come back in the
        result.  ValueError when there is neither a modality nor a table to take B from."""
        visual, tactile = x
        if cast:
            c = lambda t: None if t is None else t.to(torch.float32).contiguous()
        else:
            c = lambda t: None if t is None else t.contiguous()
        ins = [c(visual), c(tactile), c(pose) if self.use_pose else None]
        ref = next((t for t in ins if t is not None), None)
        if ref is not None:
            return ins, ref.shape[0]
        if available is None:
            raise ValueError(f"{who} needs at least one modality")
        return ins, len(available)                             # a request of prior-only rows

    @staticmethod
    def _shapes(tensors, *tag, dtype=False):
        """The shape part of a graph key: per tensor ``tag`` + (its dtype) + its shape, None for one that is not given."""
        return tuple(None if t is None else tag + ((str(t.dtype),) if dtype else ()) + tuple(t.shape) for t in tensors)

    @staticmethod
    def _count(name, value, what):
        """``value`` as an int; ValueError unless it is an integer >= 1 (no bool)."""
        if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < 1:
            raise ValueError(f"{name} must be an integer >= 1 (the number of {what}), got {value!r}")
        return int(value)

    def _decoder_row(self):
        """Elements per row of the decoders' largest activation, the last hidden layer's [rows][32][S / 2][S / 2] (32 * 32 * 32 at
        the reference's 64 x 64)."""
        return 32 * (self.model.visual_decoder.image_size // 2) ** 2

    @staticmethod
    def _fits(name, count, unit, B, per_row, tensor, largest):
        """The kernels index with 32-bit element offsets: ValueError when ``count`` * B rows of ``per_row`` elements reach 2^31."""
        if count * B * per_row >= 1 << 31:
            raise ValueError(f"{name} = {count} {unit}of B = {B} rows make a {tensor} of {count * B} x {per_row} elements, past 2^31; "
                             f"the largest {largest} for B = {B} is {((1 << 31) - 1) // (B * per_row)}")

    @torch.no_grad()
    def forward(self, x, pose=None, condition=None, available=None):
        """``MVAE.forward`` semantics: x = [visual | None, tactile | None]; returns (visual_recon, tactile_recon,
        pose_recon | None, means, log_var) -- logits, like the reference.  ``condition`` (conditional models; ValueError when it
        is missing, or given to an unconditional model): [B, condition_dim] real values, or class indices [B] / [B,1] of any
        integer dtype for a categorical model.  It is a static input of the captured graph -- the key carries its shape and
        kind -- so a replay with a new condition of the same shape gives that condition's result.  An index outside
        [0, condition_dim) is served as an all-zero condition block and reported by :meth:`bad_condition`; forward itself does
        not synchronise.  The returned tensors are the graph's static outputs: copy them if they must survive the next call with
        the same shapes.

        ``available`` (optional): a MIXED request -- [B, 2] (visual, tactile: what the dataset yields per frame) or [B, 3]
        (+ pose), any bool / integer / floating dtype, non-zero = present; with [B, 2] the pose is present wherever a pose tensor
        is given; a modality passed as ``None`` is absent in every row.  Row b is served from the modalities row b holds (none:
        the prior alone), bitwise as a whole-batch request of that subset would serve it; the tensors of an absent (row, modality)
        may hold anything finite.  The table is one more static input of the captured graph: the key carries its presence, not
        its contents, so one graph serves every mixture of a batch shape, with the launches of the joint request (the PoE launch
        is replaced one for one).  The values are not inspected and nothing synchronises; wrong shape / dtype: ValueError."""
        ins, B = self._request("forward", x, pose, available)
        cond = self._condition(condition, B)
        key = ("fwd",) + self._shapes(ins) + (self._cond_key(cond),)
        if available is None:
            return self._run(key, self._forward, ins + [cond])
        avail = self._availability(available, B)
        return self._run(key + self._shapes([avail], "avail"), self._forward, ins + [cond, avail])

    __call__ = forward

    def _score(self, self_target, visual, tactile, pose, tv, tt, tp, mask, cond=None, avail=None, tavail=None):
        """One forward of the given subset, then the per-sample terms of that pass: the row kernels on the logits, the pose
        reconstruction and the posterior the forward left on the device.  Tables (fp64 [2][B], zeroed by a fill that a captured
        graph replays): bce = (visual, tactile), mse = (pose, 0), kl = (KL, 0); the assembly adds the two rows of each table."""
        v, t, pr, mu, lv = self._forward(visual, tactile, pose, cond, avail)
        if self_target:
            tv, tt, tp = visual, tactile, pose if self.use_pose else None
        B = mu.shape[0]
        bce, mse, kl = torch.zeros(3, 2, B, dtype=torch.float64, device=mu.device)
        rows = self._score_tail(v, t, pr, mu, lv, tv, tt, tp, mask, tavail, bce, mse, kl)
        return {"rows": rows, **self._terms((bce[0], bce[1], mse[0]), (tv, tt, tp), (v, t, pr)), "kl": kl[0], "means": mu, "log_var": lv}

    def _terms(self, tables, targets, recon=None):
        """The per-term part of a result dict: each term's table, None for a term without a target; with ``recon`` = (visual
        logits, tactile logits, pose output) also ``recon_x``."""
        res = {k: tab if tg is not None else None for k, tab, tg in zip(("bce_visual", "bce_tactile", "mse_pose"), tables, targets)}
        if recon is not None:
            res["recon_x"] = list(recon[:2]) + ([recon[2]] if self.use_pose else [])
        return res

    def _row_terms(self, G, B, v, t, pr, tv, tt, tp, mask, tables):
        """The row kernels with G passes of B rows against the one target: pass g reads rows [g * B, (g + 1) * B) of the logits / the
        pose output and adds into slot g of ``tables`` = (visual, tactile, pose), each fp64 [G][B] and zeroed; ops.ROW_GROUPS_MAX
        passes per launch.  A term without a target is left out."""
        chw, hw = v[0].numel(), v[0, 0].numel()
        mc = 1 if mask is None else mask.shape[1]
        for g0 in range(0, G, ops.ROW_GROUPS_MAX):
            slots = list(range(g0, min(G, g0 + ops.ROW_GROUPS_MAX)))
            rows_of = slice(g0 * B, (slots[-1] + 1) * B)
            for lg, tg, tab in ((v, tv, tables[0]), (t, tt, tables[1])):
                if tg is not None:
                    ops.B.bce_logits_rows_groups(lg[rows_of], tg, tab, slots, B, chw, mask=mask, hw=hw, mask_channels=mc)
            if tp is not None:
                ops.B.mse_rows_groups(pr[rows_of], tp, tables[2], slots, B, tp.shape[1])

    def _assemble(self, bce, mse, kl, rows, tavail, B):
        """The assembly launch of B rows from their fp64 [2][B] tables; ``tavail``: its sibling -- a (row, term) whose target is absent
        leaves the row sum and its table entry becomes 0."""
        if tavail is None:
            ops.B.elbo_assemble_rows(bce, mse, kl, None, rows, None, 2, B, 1.0, self._pose_multiplier, self._klw, 1)
        else:
            ops.B.elbo_assemble_rows_avail(bce, mse, kl, None, rows, None, tavail, [0, 1], [2, -1], 2, B, 1.0,
                                           self._pose_multiplier, self._klw, 1)

    def _score_tail(self, v, t, pr, mu, lv, tv, tt, tp, mask, tavail, bce, mse, kl, rows=None):
        """The row kernels and the assembly of one pass into the (zeroed) fp64 [2][B] tables of :meth:`_score`; ``rows``: the fp32 [B]
        tensor to write instead of a new one.  Returns the rows."""
        B, L = mu.shape
        chw, hw = v[0].numel(), v[0, 0].numel()
        mc = 1 if mask is None else mask.shape[1]
        for slot, (lg, tg) in enumerate(((v, tv), (t, tt))):
            if tg is not None:
                ops.B.bce_logits_rows_groups(lg, tg, bce, [slot], B, chw, mask=mask, hw=hw, mask_channels=mc)
        if tp is not None:
            ops.B.mse_rows_groups(pr, tp, mse, [0], B, tp.shape[1])
        ops.B.kl_rows(mu, lv, kl[0:1], 1, B, L)
        if rows is None:
            rows = torch.empty(B, device=mu.device)
        self._assemble(bce, mse, kl, rows, tavail, B)
        return rows

    def _iw_score(self, K, self_target, visual, tactile, pose, tv, tt, tp, mask, cond=None, avail=None, tavail=None):
        """The importance-weighted bound of K draws per row: the encoders, the heads and the PoE launch ONCE (z not requested), one
        [K][B][L] draw, one iw_latent launch (z_k and the density ratio of each draw), the decoders on the K * B rows, the row
        kernels with G = K passes against the one target (slots 0..K-1 of [K][B] tables; MMDYN_BCE_GROUPS_MAX passes per launch)
        and one assembly launch.  Tables: fp64 [3][K][B] = (visual, tactile, pose), zeroed by one fill that a captured graph
        replays."""
        iw_latent, iw_assemble_rows = ops.backend_op("iw_latent"), ops.backend_op("iw_assemble_rows")
        with self._index_scope():
            (B, dev), L = self._rows_of(visual, tactile, pose, avail), self.L
            mu, lv, _ = self._poe(self._heads(visual, tactile, pose, cond), avail, None, B, dev)
            eps = self.noise.eps((K, B, L), dev)
            self.noise.commit()
            z, ratio = torch.empty(K, B, L, device=dev), torch.empty(K, B, dtype=torch.float64, device=dev)
            iw_latent(mu, lv, eps, z, ratio, K, B, L)
            # the condition rows in [K][B] order, like z
            cond_k = None if cond is None else cond.repeat((K,) + (1,) * (cond.dim() - 1))
            v, t, pr = self._decode(z.view(K * B, L), cond_k)
        if self_target:
            tv, tt, tp = visual, tactile, pose if self.use_pose else None
        tab = torch.zeros(3, K, B, dtype=torch.float64, device=dev)
        kl = torch.empty(1, B, dtype=torch.float64, device=dev)
        self._row_terms(K, B, v, t, pr, tv, tt, tp, mask, tab)
        ops.B.kl_rows(mu, lv, kl, 1, B, L)
        rows, ess = torch.empty(B, device=dev), torch.empty(B, device=dev)
        log_w = torch.empty(K, B, dtype=torch.float64, device=dev)
        iw_assemble_rows(tab[:2] if tv is not None or tt is not None else None, tab[2] if tp is not None else None, ratio, tavail,
                         rows, ess, log_w, K, B, self._pose_multiplier, 1.0, self._klw)
        return {"rows": rows, "ess": ess, "log_w": log_w, "ratio": ratio, **self._terms(tab, (tv, tt, tp), (v, t, pr)), "kl": kl[0],
                "means": mu, "log_var": lv}

    def _targets(self, what, given, B):
        """``targets`` of :meth:`score` / ``goal`` of :meth:`plan`: [visual | None, tactile | None, pose | None] -> three contiguous
        tensors / None (the pose dropped for a model without one); ValueError for an entry that does not match the batch."""
        tg = [None if t is None else t.contiguous() for t in (list(given) + [None] * 3)[:3]]
        if not self.use_pose:
            tg[2] = None
        for t, shape in zip(tg, ((B, 3), (B, 3), (B, 7))):
            if t is not None and tuple(t.shape[:2]) != shape:
                raise ValueError(f"{what} {tuple(t.shape)} does not match the batch of {B}")
        return tg

    @staticmethod
    def _loss_mask(loss_mask, pose_term, B, who, what):
        """The request's loss mask as fp32 [B][1 or 3][H][W] (None stays None); ValueError next to a pose term or for a wrong shape."""
        if loss_mask is None:
            return None
        if pose_term:
            raise ValueError(f"loss_mask is image-shaped and cannot multiply the (B, 7) pose term ({who} without a pose {what})")
        if loss_mask.dim() == 3:
            loss_mask = loss_mask.unsqueeze(1)
        if loss_mask.dim() != 4 or loss_mask.shape[0] != B or loss_mask.shape[1] not in (1, 3):
            raise ValueError(f"loss_mask {tuple(loss_mask.shape)} is not [B={B}][1 or 3][H][W]")
        return loss_mask.to(torch.float32).contiguous()

    def _set_weights(self, kl_weight, pose_multiplier):
        """The KL weight into device memory (one captured graph serves every weight) and the pose multiplier of the request."""
        if getattr(self, "_klw", None) is None:
            self._klw = torch.zeros(1, device=self.dev)
        self._klw.fill_(float(kl_weight))
        self._pose_multiplier = float(pose_multiplier)

    @torch.no_grad()
    def score(self, x, pose=None, targets=None, loss_mask=None, kl_weight=1.0, pose_multiplier=1000.0, condition=None,
              available=None, target_available=None, samples=None):
        """Per-sample terms of ONE eval-mode forward of the modality subset ``x = [visual | None, tactile | None]`` (+ ``pose``)
        against ``targets = [visual | None, tactile | None, pose | None]`` (default: the inputs that were given): a dict of
        device tensors, all ``[B]`` -- ``bce_visual`` / ``bce_tactile`` (sum over (C, H, W) of BCE-with-logits; with ``loss_mask``
        [B][1 or 3][H][W] both operands are multiplied by it first, problems.py:445-447), ``mse_pose`` (sum of the 7 squared
        differences), ``kl`` (each sample's own KL; fp64) and ``rows`` = bce_visual + bce_tactile + pose_multiplier * mse_pose +
        kl_weight * kl (fp32; a term without a target is left out and its entry is None) -- plus ``recon_x`` / ``means`` /
        ``log_var`` of the pass.  Captured and replayed under a key of its own like :meth:`forward`; the tensors are the graph's
        static outputs: copy them if they must survive the next call with the same shapes.  Forward only.  ``condition``: as in
        :meth:`forward` (required by a conditional model).

        ``available``: the inputs' per-row availability, as in :meth:`forward`.  ``target_available`` (same forms): which
        targets exist per row; it defaults to ``available`` when the targets default to the inputs, and to "all present" when
        explicit targets are given.  A (row, term) without an available target adds nothing to ``rows`` and its entry in
        ``bce_visual`` / ``bce_tactile`` / ``mse_pose`` is 0 (the assembly launch does both; no launch is added); ``kl`` is
        every row's own KL as before.

        ``samples`` (None: everything above, launch for launch): an int K >= 1 asks for the importance-weighted bound of K draws
        per row, ``rows[b] = -(logsumexp_k log_w[k][b] - log K)`` with ``log_w_k = -rec_k - kl_weight * ratio_k``: z_k = eps_k *
        exp(log_var / 2) + means for ONE [K][B][L] draw, ratio_k = log q(z_k|x) - log p(z_k) = sum 0.5 (z^2 - eps^2 - log_var)
        (its mean over draws is ``kl``), rec_k the reconstruction terms of draw k.  A loss like ``rows`` above -- equal in
        expectation at K = 1, a tighter bound on -log p(x) as K grows.  The encoders run once, the decoders on K * B rows; the
        launch count does not depend on K up to MMDYN_BCE_GROUPS_MAX = 8 draws (beyond: one more launch per term and 8 draws).
        The dict then holds ``rows`` and ``ess`` (the effective sample size of the weights, in [1, K]: how far ``rows`` can be
        trusted), both fp32 [B]; ``log_w``, ``ratio``, ``bce_visual``, ``bce_tactile``, ``mse_pose``: fp64 [K][B] (None without a
        target, an absent (row, term) 0 in all K entries); ``kl``: the analytic KL, fp64 [B]; ``means`` / ``log_var``; ``recon_x``:
        the logits of the K * B rows, draw-major.  Captured and replayed under a key that carries K; everything else as above.
        ValueError: K < 1 or no integer, or K * B rows of the largest decoder activation reaching 2^31 elements."""
        ins, B = self._request("score", x, pose, available)
        if samples is not None:
            samples = self._count("samples", samples, "latent draws per row")
            self._fits("samples", samples, "draws ", B, self._decoder_row(), "decoder activation", "samples")
        cond = self._condition(condition, B)
        self_target = targets is None
        tg = [None] * 3 if self_target else self._targets("target", targets, B)
        loss_mask = self._loss_mask(loss_mask, (ins[2] is not None) if self_target else (tg[2] is not None), B, "score", "target")
        self._set_weights(kl_weight, pose_multiplier)
        args = ins + tg + [loss_mask]
        key = ("score", self_target, self._pose_multiplier) + self._shapes(args) + (self._cond_key(cond),)
        args = args + [cond]
        if samples is None:
            fn, tail = (lambda *a: self._score(self_target, *a)), ()
        else:
            fn, tail = (lambda *a: self._iw_score(samples, self_target, *a)), (("samples", samples),)
        if available is None and target_available is None:
            return self._run(key + tail, fn, args)
        avail = self._availability(available, B)
        if target_available is None and self_target:
            target_available = available
        tavail = self._availability(target_available, B)
        return self._run(key + self._shapes((avail, tavail), "avail") + tail, fn, args + [avail, tavail])

    def _complete(self, sample, visual, tactile, pose, cond, avail):
        """One (mixed) forward, then one select launch per returned modality."""
        v, t, pr, _, _ = self._forward(visual, tactile, pose, cond, avail, sample)
        out_v, out_t = torch.empty_like(v), torch.empty_like(t)
        ops.B.complete_select(visual, v, avail, 0, out_v, True)
        ops.B.complete_select(tactile, t, avail, 1, out_t, True)
        out_p = None
        if self.use_pose:
            out_p = torch.empty_like(pr)
            ops.B.complete_select(pose, pr, avail, 2, out_p, False)
        return out_v, out_t, out_p

    @torch.no_grad()
    def complete(self, x, pose=None, available=None, condition=None, sample=False):
        """The completed request: ``(visual, tactile, pose | None)`` in [0, 1] image space.  Rows of a modality that the request
        holds (``available`` as in :meth:`forward`; None: every given modality in every row) are the caller's inputs bit for bit;
        absent rows -- and a modality passed as ``None`` -- are the model's reconstruction from whatever that row does hold: the
        sigmoid of the decoder's logits for the images, the pose decoder's output for the pose.  ``sample=False`` decodes the
        posterior mean (eps = 0); ``sample=True`` draws from the engine's Philox stream like :meth:`forward`.  Captured and
        replayed under a key of its own: the launches of :meth:`forward` plus one select launch per returned modality.  The
        tensors are the graph's static outputs; nothing synchronises."""
        ins, B = self._request("complete", x, pose, available, cast=True)
        cond = self._condition(condition, B)
        avail = self._availability(available, B)
        sample = bool(sample)
        key = ("complete", sample) + self._shapes(ins) + (self._cond_key(cond),) + self._shapes([avail], "avail")
        return self._run(key, lambda *a: self._complete(sample, *a), ins + [cond, avail])

    def _candidates(self, candidates, B):
        """The request's candidate conditions laid out candidate-major for the kernels: (fp32 [N * B][condition_dim], or int64
        [N * B] for a categorical model; N; whether they were given per row).  A few torch ops on a tiny tensor, before the captured
        region; the values are not looked at."""
        cd = self.condition_dim
        if self.categorical:
            if candidates is None:
                candidates = torch.arange(cd)
            from .models.vae import _INDEX_DTYPES
            if not torch.is_tensor(candidates) or candidates.dtype not in _INDEX_DTYPES:
                raise ValueError("categorical candidates are class indices of an integer dtype, [N] or [B, N]; got "
                                 f"{candidates.dtype if torch.is_tensor(candidates) else type(candidates).__name__}")
            per_row = candidates.dim() == 2
            if candidates.dim() not in (1, 2) or (per_row and candidates.shape[0] != B):
                raise ValueError(f"categorical candidates are [N] (shared) or [B={B}, N] (per row), got {tuple(candidates.shape)}")
            N = candidates.shape[-1]
            c = candidates.detach().to(device=self.dev, dtype=torch.int64)
            rows = (c.t() if per_row else c.unsqueeze(1).expand(N, B)).reshape(N * B)
        else:
            if not torch.is_tensor(candidates) or not candidates.dtype.is_floating_point:
                raise ValueError(f"real-valued candidates are a floating-point tensor [N, {cd}] or [B, N, {cd}], got "
                                 f"{candidates.dtype if torch.is_tensor(candidates) else type(candidates).__name__}")
            per_row = candidates.dim() == 3
            if candidates.dim() not in (2, 3) or candidates.shape[-1] != cd or (per_row and candidates.shape[0] != B):
                raise ValueError(f"real-valued candidates are [N, {cd}] (shared) or [B={B}, N, {cd}] (per row), got "
                                 f"{tuple(candidates.shape)}")
            N = candidates.shape[-2]
            c = candidates.detach().to(device=self.dev, dtype=torch.float32)
            rows = (c.transpose(0, 1) if per_row else c.unsqueeze(1).expand(N, B, cd)).reshape(N * B, cd)
        if N < 1:
            raise ValueError("plan needs at least one candidate condition (N >= 1)")
        return rows.contiguous(), N, per_row

    def _plan_candidates(self, N, sample, visual, tactile, pose, gv, gt, gp, mask, cand, avail, tavail):
        """The encoder trunks (and the pose heads) ONCE on the B rows; the image heads, the PoE launch and the decoders on the N * B
        (candidate, row) rows, candidate-major; the row kernels with G = N passes against the one goal (slots 0..N-1 of [N][B]
        tables, ops.ROW_GROUPS_MAX passes per launch); one plan_select and one gather_best launch.  Tables: fp64 [3][N][B] =
        (visual, tactile, pose), zeroed by one fill that a captured graph replays."""
        plan_select, gather_best = ops.backend_op("plan_select"), ops.backend_op("gather_best")
        ops.backend_op("concat_condition_tiled")        # (a backend without the join: an error before anything is launched)
        with self._index_scope():
            (B, dev), L = self._rows_of(visual, tactile, pose, avail), self.L
            heads = self._heads(visual, tactile, pose, cand, x_rows=B)
            if heads[2] is not None:
                heads[2] = heads[2].repeat(N, 1)
            eps = (self._draw_latent(B) if sample else self._zero_latent(B)).repeat(N, 1)       # one draw per row, shared by its candidates
            mu, lv, z = self._poe(heads, None if avail is None else avail.repeat(N, 1), eps, N * B, dev)
            v, t, pr = self._decode(z, cand)
        tab = torch.zeros(3, N, B, dtype=torch.float64, device=dev)
        kl = torch.empty(N, B, dtype=torch.float64, device=dev)
        self._row_terms(N, B, v, t, pr, gv, gt, gp, mask, tab)
        ops.B.kl_rows(mu, lv, kl.view(1, N * B), 1, N * B, L)
        cost, best, best_cost = torch.empty(N, B, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev)
        best_cond = torch.empty((B,) + tuple(cand.shape[1:]), dtype=cand.dtype, device=dev)
        plan_select(tab[:2] if gv is not None or gt is not None else None, tab[2] if gp is not None else None, kl, tavail, cand,
                    cost, best, best_cost, best_cond, N, B, self._pose_multiplier, 1.0, self._klw)
        groups = [{"src": v, "out": torch.empty((B,) + tuple(v.shape[1:]), device=dev), "logits": True},
                  {"src": t, "out": torch.empty((B,) + tuple(t.shape[1:]), device=dev), "logits": True}]
        if self.use_pose:
            groups.append({"src": pr, "out": torch.empty(B, pr.shape[1], device=dev), "logits": False})
        gather_best(groups, best, N, B)
        return {"cost": cost, "best": best, "best_cost": best_cost, "best_condition": best_cond,
                "prediction": [g["out"] for g in groups] + ([] if self.use_pose else [None]),
                **self._terms(tab, (gv, gt, gp), (v, t, pr)), "kl": kl, "means": mu.view(N, B, L), "log_var": lv.view(N, B, L)}

    @torch.no_grad()
    def plan(self, x, pose=None, goal=None, candidates=None, loss_mask=None, kl_weight=0.0, pose_multiplier=1000.0, available=None,
             goal_available=None, sample=False):
        """The inverse question of a conditional model: given the state ``x`` (+ ``pose``, ``available``: as in :meth:`forward`)
        and a ``goal`` state, which of N candidate conditions gets there?  Every candidate is scored against the goal and the best
        one is picked on the device, in ONE captured graph: the encoder trunks run once on the B rows, the image heads, the PoE
        launch and the decoders on the N * B (candidate, row) rows, and the launch count does not depend on N up to
        MMDYN_BCE_GROUPS_MAX = 8 candidates (beyond: one more launch per term and 8 candidates).

        ``goal`` = [visual | None, tactile | None, pose | None] with at least one entry, shapes as the targets of :meth:`score`;
        ``goal_available`` / ``loss_mask``: as ``target_available`` / ``loss_mask`` there.  ``candidates``: fp [N, condition_dim]
        (shared by every row) or [B, N, condition_dim] (per row); for a categorical model class indices of any integer dtype, [N] or
        [B, N], None = every class 0 .. condition_dim-1.  They are a static input of the graph: the key carries N and the kind, not
        the values.  An index outside [0, condition_dim) is served as an all-zero block and reported by :meth:`bad_condition`.
        ``sample=False``: z = the posterior mean of each (candidate, row), deterministic; ``sample=True``: ONE [B, L] draw from the
        engine's Philox stream, shared by the N candidates of a row (common random numbers: candidates differ only through the
        condition).

        cost[n][b] = bce_visual + bce_tactile + pose_multiplier * mse_pose + kl_weight * kl of candidate n's prediction for row b
        against the goal, in fp64 in that order; a term without a goal, and an absent (row, term) under ``goal_available``, is left
        out (its table entries are 0).  The smallest cost wins, ties go to the lowest n, a NaN cost never wins, +-Inf are ordinary
        values; all N costs NaN: best = -1, best_cost = NaN, the row's best_condition and prediction NaN (-1 for a categorical
        model's best_condition).  The KL weight is read from device memory: one graph serves every weight.

        Returns a dict of the graph's static outputs (copy what must survive the next call of the same shapes): ``cost`` fp32
        [N, B]; ``best`` int32 [B]; ``best_cost`` fp32 [B]; ``best_condition`` fp32 [B, condition_dim] (categorical: int64 [B]);
        ``prediction`` = [visual, tactile, pose | None], the winner's next state [B, ...] -- images in image space (sigmoid), the
        pose plain, what :meth:`rollout` / :meth:`complete` would feed on; ``bce_visual`` / ``bce_tactile`` / ``mse_pose`` (fp64
        [N, B], None without a goal), ``kl`` (fp64 [N, B]); ``means`` / ``log_var`` [N, B, L]; ``recon_x``: the logits of the N * B
        rows, candidate-major.  Nothing synchronises.  ValueError: an unconditional model, no goal, N < 1, wrong shapes or dtypes,
        or N * B rows of the largest decoder activation reaching 2^31 elements."""
        if not self.conditional:
            raise ValueError("candidate conditions were passed to an unconditional model")
        ins, B = self._request("plan", x, pose, available)
        cand, N, per_row = self._candidates(candidates, B)
        self._fits("candidates", N, "conditions ", B, self._decoder_row(), "decoder activation", "N")
        if not isinstance(goal, (list, tuple)) or len(goal) > 3:
            raise ValueError("goal must be a list [visual | None, tactile | None, pose | None]")
        tg = self._targets("goal", goal, B)
        if all(t is None for t in tg):
            raise ValueError("plan needs a goal: at least one of [visual, tactile, pose]")
        loss_mask = self._loss_mask(loss_mask, tg[2] is not None, B, "plan", "goal")
        self._set_weights(kl_weight, pose_multiplier)
        sample = bool(sample)
        avail, tavail = self._availability(available, B), self._availability(goal_available, B)
        args = ins + tg + [loss_mask, cand, avail, tavail]
        key = ("plan",) + self._shapes(ins + tg + [loss_mask]) + \
            ("index" if self.categorical else "real", ("candidates", N, per_row), sample, self._pose_multiplier) + \
            self._shapes((avail, tavail), "avail")
        return self._run(key, lambda *a: self._plan_candidates(N, sample, *a), args)

    def _candidate_steps(self, candidates, B, T):
        """The request's candidate condition SEQUENCES laid out step-major and candidate-major for the kernels: (fp32
        [T][N * B][condition_dim], or int64 [T][N * B] for a categorical model; N; whether they were given per row).  A few torch ops
        on a tiny tensor, before the captured region; the values are not looked at."""
        cd = self.condition_dim
        if self.categorical:
            from .models.vae import _INDEX_DTYPES
            if not torch.is_tensor(candidates) or candidates.dtype not in _INDEX_DTYPES:
                raise ValueError("categorical candidates are class indices of an integer dtype, [N, T] or [B, N, T]; got "
                                 f"{candidates.dtype if torch.is_tensor(candidates) else type(candidates).__name__}")
            per_row = candidates.dim() == 3
            if candidates.dim() not in (2, 3) or candidates.shape[-1] != T or (per_row and candidates.shape[0] != B):
                raise ValueError(f"categorical candidates are [N, T={T}] (shared) or [B={B}, N, T={T}] (per row), got "
                                 f"{tuple(candidates.shape)}")
            N = candidates.shape[-2]
            c = candidates.detach().to(device=self.dev, dtype=torch.int64)
            rows = (c.permute(2, 1, 0) if per_row else c.t().unsqueeze(2).expand(T, N, B)).reshape(T, N * B)
        else:
            if not torch.is_tensor(candidates) or not candidates.dtype.is_floating_point:
                raise ValueError(f"real-valued candidates are a floating-point tensor [N, T, {cd}] or [B, N, T, {cd}], got "
                                 f"{candidates.dtype if torch.is_tensor(candidates) else type(candidates).__name__}")
            per_row = candidates.dim() == 4
            if candidates.dim() not in (3, 4) or candidates.shape[-1] != cd or candidates.shape[-2] != T or \
                    (per_row and candidates.shape[0] != B):
                raise ValueError(f"real-valued candidates are [N, T={T}, {cd}] (shared) or [B={B}, N, T={T}, {cd}] (per row), got "
                                 f"{tuple(candidates.shape)}")
            N = candidates.shape[-3]
            c = candidates.detach().to(device=self.dev, dtype=torch.float32)
            rows = (c.permute(2, 1, 0, 3) if per_row else c.transpose(0, 1).unsqueeze(2).expand(T, N, B, cd)).reshape(T, N * B, cd)
        if N < 1:
            raise ValueError("plan_rollout needs at least one candidate condition sequence (N >= 1)")
        return rows.contiguous(), N, per_row

    def _candidate_steps_forward(self, N, T, Tg, sample, B, dev, step0_heads, cand, avail_rows, gv, gt, gp, traj, means, log_var, tab):
        """The step loop of the horizon planner on the N * B (candidate, row) rows, shared by :meth:`_plan_rollout` and
        :meth:`_plan_refine`: step 0's heads come from ``step0_heads(cand[0])`` (the trunks on the B rows, the image heads through the
        tiled join), every later step is the joint forward of the N * B state rows with the step's slice of ``cand``; PoE writes
        slot t of ``means`` / ``log_var``, ONE rollout_feed slot t of the ``traj`` tensors, a scored step adds the row kernels and
        kl_rows into ``tab`` (fp64 [4][Tg][N][B], cleared by the caller).  ``avail_rows``: the request's table on the N * B rows."""
        feed = ops.backend_op("rollout_feed")
        NB, L, kl = N * B, self.L, tab[3]
        step_of = lambda t, i: None if t is None else t[i]
        state = None
        for i in range(T):
            c_i = cand[i]
            heads = step0_heads(c_i) if i == 0 else self._heads(state[0], state[1], state[2], c_i)
            # one draw per row and step, shared by the row's candidates
            eps = (self._draw_latent(B) if sample else self._zero_latent(B)).repeat(N, 1)
            mu, lv, z = self._poe(heads, avail_rows if i == 0 else None, eps, NB, dev, out=(means[i], log_var[i]))
            v, t, pr = self._decode(z, c_i)
            if Tg == T or i == T - 1:
                s = i if Tg == T else 0
                self._row_terms(N, B, v, t, pr, step_of(gv, s), step_of(gt, s), step_of(gp, s), None, (tab[0, s], tab[1, s], tab[2, s]))
                ops.B.kl_rows(mu, lv, kl[s].view(1, NB), 1, NB, L)
            groups = [{"recon": v, "obs": None, "out": traj[0][i], "logits": True, "column": 0},
                      {"recon": t, "obs": None, "out": traj[1][i], "logits": True, "column": 1}]
            if self.use_pose:
                groups.append({"recon": pr, "obs": None, "out": traj[2][i], "logits": False, "column": 2})
            feed(groups, None, NB)
            state = [traj[0][i], traj[1][i], traj[2][i] if self.use_pose else None]

    def _plan_rollout(self, N, T, Tg, sample, top, visual, tactile, pose, gv, gt, gp, cand, avail, tavail, weight):
        """N candidate condition sequences per row rolled out open loop over T steps on the N * B (candidate, row) rows.  Step 0 is
        the front half of :meth:`_plan_candidates` (the trunks and the pose heads ONCE on the B rows, the image heads through the
        tiled join, PoE and the decoders on N * B rows); every later step is the joint forward of the N * B state rows with the
        step's slice of the candidates; ONE rollout_feed per step writes slot t of the [T][N * B][...] trajectory tensors, which the
        next step reads.  A scored step (the last one for a final goal, Tg = 1; every one for Tg = T) adds the row kernels with G = N
        passes against its one goal and kl_rows; tables fp64 [4][Tg][N][B] = (visual, tactile, pose, KL), cleared by one fill.  One
        plan_select_steps and one gather_best_steps launch close the request."""
        select, gather = ops.backend_op("plan_select_steps"), ops.backend_op("gather_best_steps")
        ops.backend_op("rollout_feed")
        ops.backend_op("concat_condition_tiled")        # (a backend without the join: an error before anything is launched)
        (B, dev), L, S = self._rows_of(visual, tactile, pose, avail), self.L, self.model.visual_decoder.image_size
        NB = N * B
        traj = [torch.empty(T, NB, 3, S, S, device=dev), torch.empty(T, NB, 3, S, S, device=dev),
                torch.empty(T, NB, 7, device=dev) if self.use_pose else None]
        means, log_var = torch.empty(T, NB, L, device=dev), torch.empty(T, NB, L, device=dev)
        tab = torch.zeros(4, Tg, N, B, dtype=torch.float64, device=dev)
        kl = tab[3]

        def step0(c_0):
            heads = self._heads(visual, tactile, pose, c_0, x_rows=B)
            if heads[2] is not None:
                heads[2] = heads[2].repeat(N, 1)
            return heads
        with self._index_scope():
            self._candidate_steps_forward(N, T, Tg, sample, B, dev, step0, cand, None if avail is None else avail.repeat(N, 1),
                                          gv, gt, gp, traj, means, log_var, tab)
        cost, step_cost = torch.empty(N, B, device=dev), torch.empty(Tg, N, B, device=dev)
        best, best_cost = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev)
        best_cond = torch.empty((B, T) + tuple(cand.shape[2:]), dtype=cand.dtype, device=dev)
        top_idx = top_cost = None
        if top is not None:
            top_idx, top_cost = torch.empty(top, B, dtype=torch.int32, device=dev), torch.empty(top, B, device=dev)
        select(tab[:2] if gv is not None or gt is not None else None, tab[2] if gp is not None else None, kl, tavail, weight, cand,
               cost, step_cost, best, best_cost, best_cond, top_idx, top_cost, N, B, T, Tg, self._pose_multiplier, 1.0, self._klw)
        outs = [{"src": x, "out": torch.empty((T, B) + tuple(x.shape[2:]), device=dev), "logits": False} for x in traj if x is not None]
        gather(outs, best, N, B, T)
        split = lambda x: None if x is None else x.view((T, N, B) + tuple(x.shape[2:]))
        res = {"cost": cost, "step_cost": step_cost, "best": best, "best_cost": best_cost, "best_condition": best_cond,
               "trajectory": [g["out"] for g in outs] + ([] if self.use_pose else [None]),
               "visual": split(traj[0]), "tactile": split(traj[1]), "pose": split(traj[2]),
               **self._terms(tab[:3], (gv, gt, gp)), "kl": kl, "means": split(means), "log_var": split(log_var)}
        if top is not None:
            res.update(top=top_idx, top_cost=top_cost)
        return res

    def _horizon_goal(self, who, goal, goal_available, step_weight, T, B):
        """The goal of a horizon request: (the three goal tensors as fp32 [Tg, B, ...] / None, the goal-availability tables uint8
        [Tg][B][4] / None, the step weights fp32 [Tg] on the device / None, Tg); ValueError for what :meth:`plan_rollout` refuses."""
        if not isinstance(goal, (list, tuple)) or len(goal) > 3:
            raise ValueError("goal must be a list [visual | None, tactile | None, pose | None]")
        goal = (list(goal) + [None] * 3)[:3]
        if not self.use_pose:
            goal[2] = None
        given = [(i, t) for i, t in enumerate(goal) if t is not None]
        if not given:
            raise ValueError(f"{who} needs a goal: at least one of [visual, tactile, pose]")
        if not all(torch.is_tensor(t) for _, t in given):
            raise ValueError("goal must hold tensors")
        # an image [B, 3, S, S] / a pose [B, 7] is a final goal, one more leading dimension a goal per step
        forms = {t.dim() - (4 if i < 2 else 2) for i, t in given}
        if not forms <= {0, 1}:
            raise ValueError("goal tensors are [B, ...] (a final goal) or [T, B, ...] (one per step)")
        if len(forms) > 1:
            raise ValueError("goal mixes the two forms: every tensor is [B, ...] (a final goal) or every one [T, B, ...] (one per step)")
        Tg = 1 if forms == {0} else T
        if forms == {0}:
            tg = [None if t is None else t.to(device=self.dev, dtype=torch.float32).unsqueeze(0)
                  for t in self._targets("goal", goal, B)]
            tavail = self._availability(goal_available, B)
            tavail = None if tavail is None else tavail.view(1, B, -1)
        else:
            tg = self._step_tensors("goal", goal, T, B)
            tavail = self._step_availability("goal_available", goal_available, T, B)
        weight = None
        if step_weight is not None:
            if not torch.is_tensor(step_weight) or not step_weight.dtype.is_floating_point or tuple(step_weight.shape) != (Tg,):
                raise ValueError(f"step_weight must be a floating-point tensor [Tg={Tg}] (one weight per scored step), got "
                                 f"{tuple(step_weight.shape) if torch.is_tensor(step_weight) else type(step_weight).__name__}")
            weight = step_weight.detach().to(device=self.dev, dtype=torch.float32).contiguous()
        return tg, tavail, weight, Tg

    @torch.no_grad()
    def plan_rollout(self, x, pose=None, steps=1, goal=None, candidates=None, step_weight=None, top=None, kl_weight=0.0,
                     pose_multiplier=1000.0, available=None, goal_available=None, sample=False):
        """:meth:`plan` over a horizon: which of N candidate condition SEQUENCES takes the state ``x`` (+ ``pose``, ``available``:
        as in :meth:`forward`) to the goal over the next ``steps`` = T applications of the model?  Every sequence is rolled out open
        loop (:meth:`rollout` with nothing observed) on the N * B (candidate, row) rows, scored against the goal, and the best one
        is picked on the device together with its trajectory -- ONE captured graph, the random-shooting planner of model-predictive
        control.  Step 0 runs the encoder trunks once on the B rows (the image heads, the PoE launch and the decoders on N * B
        rows); every later step is the joint forward of the N * B state rows under the step's conditions.

        ``candidates`` (required): fp [N, T, condition_dim] (shared by every row) or [B, N, T, condition_dim] (per row); for a
        categorical model class indices of any integer dtype, [N, T] or [B, N, T].  A static input of the graph: the key carries N,
        T, the kind and whether they are per row, never the values; :meth:`bad_condition` covers the whole call.  ``goal`` =
        [visual | None, tactile | None, pose | None] with at least one entry; every given tensor [B, ...] -- a FINAL goal, only
        step T-1 is scored (Tg = 1) -- or every one [T, B, ...] -- every step is scored against its own goal (Tg = T);
        ``goal_available``: [B, 2 | 3] or [T, B, 2 | 3] to match, in the forms ``target_available`` of :meth:`score` takes.  An
        unscored step issues no row kernel.  ``step_weight``: fp [Tg] or None (all ones); it lives in device memory, its values
        are never looked at (NaN / Inf propagate).  ``sample=False`` decodes posterior means; ``sample=True`` draws ONE [B, L]
        block per step from the engine's Philox stream, shared by the N candidates of a row (common random numbers, as in
        :meth:`plan`); the stream advances as :meth:`rollout`'s does.

        step_cost[t][n][b] = the cost of :meth:`plan` for step t of candidate n, in fp64; cost[n][b] = sum_t step_weight[t] *
        step_cost[t][n][b] in fp64, t ascending.  The smallest total wins under the rules of :meth:`plan` (ties: the lowest n; a
        NaN total never wins; all NaN: best = -1, NaN outputs).  ``top`` = K in [1, MMDYN_PLAN_TOP_MAX = 8] also returns the K best
        candidates per row in ascending order (the building block of iterative refitting; -1 / NaN past the non-NaN candidates).

        Returns a dict of the graph's static outputs (copy what must survive the next call of the same shapes): ``cost`` fp32
        [N, B]; ``step_cost`` fp32 [Tg, N, B]; ``best`` int32 [B]; ``best_cost`` fp32 [B]; ``best_condition`` fp32 [B, T,
        condition_dim] (categorical: int64 [B, T]); ``trajectory`` = [visual, tactile, pose | None], the winner's states [T, B, ...]
        (slot t = s_{t+1}, image space); ``visual`` / ``tactile`` / ``pose``: all states, [T, N, B, ...]; ``bce_visual`` /
        ``bce_tactile`` / ``mse_pose`` (fp64 [Tg, N, B], None without that goal; an absent (step, row, term) is 0) and ``kl`` (fp64
        [Tg, N, B]); ``means`` / ``log_var`` [T, N, B, L]; with ``top``: ``top`` int32 [K, B] and ``top_cost`` fp32 [K, B].  Nothing
        synchronises.  ValueError: an unconditional model, no goal, goals of both forms, N < 1, ``steps`` no integer >= 1, wrong
        shapes or dtypes, ``top`` outside [1, 8], or a trajectory tensor / the decoders' largest N * B-row activation reaching 2^31
        elements.  Out of scope: observations inside a plan, ``loss_mask``."""
        if not self.conditional:
            raise ValueError("candidate conditions were passed to an unconditional model")
        T = self._count("steps", steps, "model applications")
        ins, B = self._request("plan_rollout", x, pose, available, cast=True)
        cand, N, per_row = self._candidate_steps(candidates, B, T)
        S = self.model.visual_decoder.image_size
        most = min(((1 << 31) - 1) // (T * B * 3 * S * S), ((1 << 31) - 1) // (B * self._decoder_row()))
        if N > most:
            raise ValueError(f"candidates = {N} condition sequences of B = {B} rows over steps = {T} make a trajectory tensor or a "
                             f"decoder activation of 2^31 elements or more; the largest N for B = {B} and steps = {T} is {most}")
        if top is not None:
            if isinstance(top, bool) or not isinstance(top, numbers.Integral) or not 1 <= top <= ops.PLAN_TOP_MAX:
                raise ValueError(f"top must be an integer in [1, {ops.PLAN_TOP_MAX}] (the best candidates listed per row), got {top!r}")
            top = int(top)
        tg, tavail, weight, Tg = self._horizon_goal("plan_rollout", goal, goal_available, step_weight, T, B)
        self._set_weights(kl_weight, pose_multiplier)
        sample = bool(sample)
        avail = self._availability(available, B)
        args = ins + tg + [cand, avail, tavail, weight]
        key = ("plan_rollout", T, Tg, top, sample, self._pose_multiplier, "index" if self.categorical else "real",
               ("candidates", N, per_row)) + self._shapes(ins + tg + [weight]) + self._shapes((avail, tavail), "avail")
        return self._run(key, lambda *a: self._plan_rollout(N, T, Tg, sample, top, *a), args)

    def _plan_refine(self, N, K, I, T, Tg, sample, alpha, std_min, temperature, warm, visual, tactile, pose, gv, gt, gp, init_mean,
                     init_std, lo, hi, avail, tavail, weight, prev_mean=None, prev_std=None, prev_keep=None):
        """The cross-entropy method on the horizon planner, I iterations in one captured region.  Once per request: the trunks and
        the pose heads on the B rows (:meth:`_trunks`).  Per iteration: one [N][B][T][cd] draw and its commit, one plan_sample (slot
        0 = the previous iteration's winner), one fill of the tables, the steps of :meth:`_plan_rollout` from the image heads on,
        one plan_select_steps and one plan_refit (in place from the second iteration on).  Every buffer is allocated once; the
        winner's cost and the elite count of iteration i are written straight into row i of ``history`` / ``elite_count``.  One
        gather_best_steps on the last iteration's trajectories closes the request.  ``temperature`` (MPPI): every refit is
        plan_refit_weighted, which also writes row i of ``ess`` and the [N][B] weights.  ``warm`` = (shift, widen): one plan_shift in
        front of the loop writes ``mean`` / ``std`` and the incumbent of round 0 from the previous plan; round 0 then samples from
        them and refits in place."""
        select, gather, sample_op, refit = (ops.backend_op(k) for k in ("plan_select_steps", "gather_best_steps", "plan_sample",
                                                                        "plan_refit" if temperature is None else "plan_refit_weighted"))
        shift_op = None if warm is None else ops.backend_op("plan_shift")
        ops.backend_op("rollout_feed")
        ops.backend_op("concat_condition_tiled")        # (a backend without the join: an error before anything is launched)
        (B, dev), L, S, cd = self._rows_of(visual, tactile, pose, avail), self.L, self.model.visual_decoder.image_size, self.condition_dim
        NB = N * B
        traj = [torch.empty(T, NB, 3, S, S, device=dev), torch.empty(T, NB, 3, S, S, device=dev),
                torch.empty(T, NB, 7, device=dev) if self.use_pose else None]
        means, log_var = torch.empty(T, NB, L, device=dev), torch.empty(T, NB, L, device=dev)
        tab = torch.empty(4, Tg, N, B, dtype=torch.float64, device=dev)
        kl = tab[3]
        cand = torch.empty(T, NB, cd, device=dev)
        mean, std = torch.empty(B, T, cd, device=dev), torch.empty(B, T, cd, device=dev)
        cost, step_cost = torch.empty(N, B, device=dev), torch.empty(Tg, N, B, device=dev)
        best, best_cond = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, T, cd, device=dev)
        history, count = torch.empty(I, B, device=dev), torch.empty(I, B, dtype=torch.int32, device=dev)
        avail_rows = None if avail is None else avail.repeat(N, 1)
        extra, keep0 = {}, None
        if temperature is not None:
            extra = {"ess": torch.empty(I, B, device=dev), "weight": torch.empty(N, B, dtype=torch.float64, device=dev)}
        if warm is not None:
            keep0 = torch.empty(B, T, cd, device=dev)
        with self._index_scope():
            trunks = self._trunks(visual, tactile, pose)
            if trunks[2] is not None:
                trunks[2] = trunks[2].repeat(N, 1)                    # the pose heads see no condition: their N * B rows once
            step0 = lambda c_0: self._heads_of(trunks, c_0, x_rows=B)
            if warm is not None:
                shift_op(prev_mean, prev_std, prev_keep, init_mean, init_std, mean, std, keep0, B, T, warm[0], warm[1])
            for i in range(I):
                eps = self.noise.eps((N, B, T, cd), dev)
                self.noise.commit()
                m_in, s_in = (init_mean, init_std) if i == 0 and warm is None else (mean, std)
                sample_op(m_in, s_in, eps, keep0 if i == 0 else best_cond, lo, hi, cand, N, B, T)
                tab.zero_()
                self._candidate_steps_forward(N, T, Tg, sample, B, dev, step0, cand, avail_rows, gv, gt, gp, traj, means, log_var, tab)
                select(tab[:2] if gv is not None or gt is not None else None, tab[2] if gp is not None else None, kl, tavail, weight,
                       cand, cost, step_cost, best, history[i], best_cond, None, None, N, B, T, Tg, self._pose_multiplier, 1.0, self._klw)
                if temperature is None:
                    refit(cost, cand, m_in, s_in, mean, std, None, count[i], K, N, B, T, alpha, std_min)
                else:
                    refit(cost, cand, m_in, s_in, mean, std, None, count[i], extra["weight"], extra["ess"][i], K, N, B, T, temperature,
                          alpha, std_min)
        outs = [{"src": x, "out": torch.empty((T, B) + tuple(x.shape[2:]), device=dev), "logits": False} for x in traj if x is not None]
        gather(outs, best, N, B, T)
        split = lambda x: None if x is None else x.view((T, N, B) + tuple(x.shape[2:]))
        return {"cost": cost, "step_cost": step_cost, "best": best, "best_cost": history[I - 1], "best_condition": best_cond,
                "trajectory": [g["out"] for g in outs] + ([] if self.use_pose else [None]),
                "visual": split(traj[0]), "tactile": split(traj[1]), "pose": split(traj[2]),
                **self._terms(tab[:3], (gv, gt, gp)), "kl": kl, "means": split(means), "log_var": split(log_var),
                "mean": mean, "std": std, "candidates": split(cand), "history": history, "elite_count": count, **extra}

    @torch.no_grad()
    def plan_refine(self, x, pose=None, steps=1, goal=None, init_mean=None, init_std=None, candidates=64, elites=8, iterations=4,
                    alpha=0.0, std_min=0.0, bounds=None, step_weight=None, kl_weight=0.0, pose_multiplier=1000.0, available=None,
                    goal_available=None, sample=False, temperature=None, warm_start=None, shift=1, widen=0.0):
        """:meth:`plan_rollout` with the candidates made and refined on the device: the cross-entropy method (CEM) over a horizon,
        for models with real-valued conditions.  A distribution N(mean, std^2) over condition sequences [T, condition_dim] per row
        starts at ``init_mean`` / ``init_std``; each of ``iterations`` = I rounds draws ``candidates`` = N sequences per row from
        it (slot 0 is the incumbent: the mean in round 0, the previous round's winner afterwards, so the best cost never gets worse
        beyond rounding), rolls them out over ``steps`` = T applications of the model exactly as :meth:`plan_rollout` does, scores
        them against the goal, and refits mean and std to the ``elites`` = K cheapest of each row:
        mean <- alpha * mean + (1 - alpha) * elite mean, std <- max(alpha * std + (1 - alpha) * elite std, std_min), the population
        standard deviation, in fp64.  ONE captured graph for all I rounds: the encoder trunks and the pose heads run once per
        request, nothing synchronises, and N may reach MMDYN_REFIT_N_MAX = 4096 with any K <= N.

        ``init_mean`` / ``init_std`` (required): floating point, [T, condition_dim] (shared by every row) or [B, T,
        condition_dim].  ``bounds`` = (lo, hi), floating point [condition_dim] each, or None: every candidate is clamped to them.
        ``goal`` / ``goal_available`` / ``step_weight`` / ``available`` / ``sample`` / the weights: as in :meth:`plan_rollout`
        (``sample=True``: one [B, L] draw per step and round, shared by a row's candidates).  All tensors are static inputs of the
        graph: its key carries I, N, K, T, the goal's form, ``sample``, ``alpha``, ``std_min``, the pose multiplier, whether
        bounds are given and the shapes -- never values.

        The Philox stream: round i draws its [N, B, T, cd] candidate block first, then (``sample=True``) the T latent blocks of its
        steps.  With n_c = ceil(N B T cd / 4), n_l = ceil(B L / 4) and per = n_c + (T n_l if sample else 0), round i of eager call c
        (on an engine that served nothing else) draws its candidates at counter (c I + i) per and the latent block of step t at
        (c I + i) per + n_c + t n_l.  The draw of slot 0 is taken and not used.  ``temperature`` and ``warm_start`` change none of
        this.

        ``temperature`` (a number > 0, rounded to fp32; None: the plain CEM above): MPPI.  Every refit weighs elite n of a row by
        w_n = exp(-(cost_n - cost_min) / temperature) in fp64 (mmdyn_plan_refit_weighted): mean and std become the weighted mean
        and the weighted population standard deviation over the ``elites`` = K cheapest; ``elites=candidates`` is pure MPPI, which
        ranks nothing.  Equal elite costs give the bits of CEM.  The result gains ``ess`` fp32 [I, B], each round's effective
        sample size (sum w)^2 / sum w^2 in [1, K'] (0 when no cost was a number), and ``weight`` fp64 [N, B], the last round's
        weights; the key gains ("mppi", temperature).

        ``warm_start`` (a mapping with ``mean``, ``std`` and ``best_condition``, floating point [B, T, condition_dim] each -- the
        dict an earlier call returned qualifies; static inputs of the graph): the receding horizon.  One mmdyn_plan_shift in front
        of the loop moves the previous plan ``shift`` steps on (an integer in [0, T]): step t of the new distribution and of round
        0's incumbent is step t + shift of the previous ``mean`` / ``std`` / ``best_condition``, the std not below ``widen`` *
        ``init_std`` (``widen`` >= 0, rounded to fp32); the last ``shift`` steps are ``init_mean`` / ``init_std`` (which stay
        required) with the incumbent at ``init_mean``.  Round 0 samples from that, so the previous winner is a candidate again.
        The key gains ("warm", shift, widen).

        Returns a dict of the graph's static outputs (copy what must survive the next call of the same shapes): everything
        :meth:`plan_rollout` returns (without ``top``), for the LAST round; ``mean`` / ``std`` fp32 [B, T, condition_dim], after the
        last refit; ``candidates`` fp32 [T, N, B, condition_dim], the last round's candidates; ``history`` fp32 [I, B], each round's
        best cost; ``elite_count`` int32 [I, B], the elites each refit found (< K when fewer costs were no NaN; 0 leaves the
        distribution as it was).  ValueError: what :meth:`plan_rollout` refuses, a categorical or unconditional model, N outside
        [1, 4096], K outside [1, N], I < 1, ``alpha`` outside [0, 1), ``std_min`` < 0, wrong shapes or dtypes of ``init_mean`` /
        ``init_std`` / ``bounds``, a ``temperature`` that is no finite number > 0 in fp32, a ``warm_start`` that is no such
        mapping, ``shift`` outside [0, T], ``widen`` < 0, or ``shift`` / ``widen`` away from their defaults without ``warm_start``.
        Out of scope: categorical distributions, observations inside a plan, ``loss_mask``, a temperature scaled by the cost
        range, weights in :meth:`plan_rollout`'s ``top``."""
        if not self.conditional:
            raise ValueError("plan_refine refits a distribution over conditions: it was asked of an unconditional model")
        if self.categorical:
            raise ValueError("plan_refine serves real-valued conditions; a distribution over the classes of a categorical model is out of scope")
        T = self._count("steps", steps, "model applications")
        N = self._count("candidates", candidates, "condition sequences drawn per row and iteration")
        K = self._count("elites", elites, "candidates each refit keeps")
        I = self._count("iterations", iterations, "refinement rounds")
        if N > ops.REFIT_N_MAX:
            raise ValueError(f"candidates = {N} is more than the refit ranks per row (MMDYN_REFIT_N_MAX = {ops.REFIT_N_MAX})")
        if K > N:
            raise ValueError(f"elites = {K} must lie in [1, candidates = {N}]")
        for name, v, ok in (("alpha", alpha, lambda a: 0.0 <= a < 1.0), ("std_min", std_min, lambda a: a >= 0.0)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not ok(float(v)):
                raise ValueError(f"{name} must be a number in {'[0, 1)' if name == 'alpha' else '[0, inf)'}, got {v!r}")
        # (as the kernel sees them: fp32)
        alpha, std_min = float(torch.tensor(float(alpha), dtype=torch.float32)), float(torch.tensor(float(std_min), dtype=torch.float32))
        if not alpha < 1.0:
            raise ValueError("alpha rounds to 1.0 in fp32: it must lie in [0, 1)")
        as_f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
        if temperature is not None:
            if isinstance(temperature, bool) or not isinstance(temperature, numbers.Real) or not 0.0 < as_f32(temperature) < float("inf"):
                raise ValueError(f"temperature must be None (CEM) or a number that is finite and > 0 in fp32 (MPPI), got {temperature!r}")
            temperature = as_f32(temperature)
        if isinstance(shift, bool) or not isinstance(shift, numbers.Integral) or not 0 <= shift <= T:
            raise ValueError(f"shift must be an integer in [0, steps = {T}] (the steps the horizon has moved on), got {shift!r}")
        if isinstance(widen, bool) or not isinstance(widen, numbers.Real) or not 0.0 <= as_f32(widen) < float("inf"):
            raise ValueError(f"widen must be a finite number >= 0 (the floor of the shifted std, in units of init_std), got {widen!r}")
        shift, widen = int(shift), as_f32(widen)
        if warm_start is None and (shift != 1 or widen != 0.0):
            raise ValueError(f"shift = {shift} and widen = {widen} move a previous plan on: they need warm_start")
        ins, B = self._request("plan_refine", x, pose, available, cast=True)
        S, cd = self.model.visual_decoder.image_size, self.condition_dim
        most = min(((1 << 31) - 1) // (T * B * 3 * S * S), ((1 << 31) - 1) // (B * self._decoder_row()))
        if N > most:
            raise ValueError(f"candidates = {N} condition sequences of B = {B} rows over steps = {T} make a trajectory tensor or a "
                             f"decoder activation of 2^31 elements or more; the largest N for B = {B} and steps = {T} is {most}")
        dist = []
        for name, t in (("init_mean", init_mean), ("init_std", init_std)):
            if not torch.is_tensor(t) or not t.dtype.is_floating_point or tuple(t.shape) not in ((T, cd), (B, T, cd)):
                raise ValueError(f"{name} must be a floating-point tensor [T={T}, {cd}] (shared) or [B={B}, T={T}, {cd}] (per row), got "
                                 f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
            dist.append(t.detach().to(device=self.dev, dtype=torch.float32).expand(B, T, cd).contiguous())
        lo = hi = None
        if bounds is not None:
            if not isinstance(bounds, (list, tuple)) or len(bounds) != 2 or not all(
                    torch.is_tensor(t) and t.dtype.is_floating_point and tuple(t.shape) == (cd,) for t in bounds):
                raise ValueError(f"bounds must be a pair (lo, hi) of floating-point tensors [{cd}] or None")
            lo, hi = (t.detach().to(device=self.dev, dtype=torch.float32).contiguous() for t in bounds)
        prev = []
        if warm_start is not None:
            if not isinstance(warm_start, collections.abc.Mapping) or not all(k in warm_start for k in ("mean", "std", "best_condition")):
                raise ValueError("warm_start must be a mapping with mean, std and best_condition (the result of an earlier plan_refine)")
            for name in ("mean", "std", "best_condition"):
                t = warm_start[name]
                if not torch.is_tensor(t) or not t.dtype.is_floating_point or tuple(t.shape) != (B, T, cd):
                    raise ValueError(f"warm_start[{name!r}] must be a floating-point tensor [B={B}, T={T}, {cd}], got "
                                     f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
                prev.append(t.detach().to(device=self.dev, dtype=torch.float32).contiguous())
        tg, tavail, weight, Tg = self._horizon_goal("plan_refine", goal, goal_available, step_weight, T, B)
        self._set_weights(kl_weight, pose_multiplier)
        sample = bool(sample)
        avail = self._availability(available, B)
        args = ins + tg + dist + [lo, hi, avail, tavail, weight] + prev
        key = ("plan_refine", I, N, K, T, Tg, sample, alpha, std_min, self._pose_multiplier, bounds is not None) + \
            self._shapes(ins + tg + dist + [weight]) + self._shapes((avail, tavail), "avail")
        if temperature is not None:
            key += (("mppi", temperature),)
        if warm_start is not None:
            key += (("warm", shift, widen),)
        warm = None if warm_start is None else (shift, widen)
        return self._run(key, lambda *a: self._plan_refine(N, K, I, T, Tg, sample, alpha, std_min, temperature, warm, *a), args)

    def _rollout(self, T, sample, per_step_cond, visual, tactile, pose, cond, avail, ov, ot, op, oav, tv, tt, tp, tav):
        """T forwards in a row, each followed by ONE feed launch that writes the next state into its trajectory slot, where the
        next step's encoders read it; with targets, the tail of :meth:`_score` per step on tables [T][3][2][B] that one fill
        clears.  Step 0 serves the request's subset / table, every later step is the joint request."""
        feed = ops.backend_op("rollout_feed")
        (B, dev), L, S = self._rows_of(visual, tactile, pose, avail), self.L, self.model.visual_decoder.image_size
        traj = [torch.empty(T, B, 3, S, S, device=dev), torch.empty(T, B, 3, S, S, device=dev),
                torch.empty(T, B, 7, device=dev) if self.use_pose else None]
        means, log_var = torch.empty(T, B, L, device=dev), torch.empty(T, B, L, device=dev)
        scoring = any(t is not None for t in (tv, tt, tp))
        if scoring:
            tab = torch.zeros(T, 3, 2, B, dtype=torch.float64, device=dev)
            rows = torch.empty(T, B, device=dev)
        state = [visual, tactile, pose]
        step_of = lambda t, i: None if t is None else t[i]
        with self._index_scope():
            for i in range(T):
                c_i = step_of(cond, i) if per_step_cond else cond
                heads = self._heads(state[0], state[1], state[2], c_i)
                eps = self._draw_latent(B) if sample else self._zero_latent(B)
                mu, lv, z = self._poe(heads, avail if i == 0 else None, eps, B, dev, out=(means[i], log_var[i]))
                v, t, pr = self._decode(z, c_i)
                if scoring:         # before the correction below: what the model predicted for frame i + 1
                    self._score_tail(v, t, pr, mu, lv, step_of(tv, i), step_of(tt, i), step_of(tp, i), None, step_of(tav, i),
                                     tab[i, 0], tab[i, 1], tab[i, 2], rows=rows[i])
                groups = [{"recon": v, "obs": step_of(ov, i), "out": traj[0][i], "logits": True, "column": 0},
                          {"recon": t, "obs": step_of(ot, i), "out": traj[1][i], "logits": True, "column": 1}]
                if self.use_pose:
                    groups.append({"recon": pr, "obs": step_of(op, i), "out": traj[2][i], "logits": False, "column": 2})
                feed(groups, step_of(oav, i), B)
                state = [traj[0][i], traj[1][i], traj[2][i] if self.use_pose else None]
        res = {"visual": traj[0], "tactile": traj[1], "pose": traj[2], "means": means, "log_var": log_var,
               "bce_visual": None, "bce_tactile": None, "mse_pose": None, "kl": None, "rows": None}
        if scoring:
            res.update(self._terms((tab[:, 0, 0], tab[:, 0, 1], tab[:, 1, 0]), (tv, tt, tp)), kl=tab[:, 2, 0], rows=rows)
        return res

    @staticmethod
    def _quantile_index(quantiles, N):
        """The order statistics of the ``linear`` quantile: h = q (N - 1) in fp64, lo = floor(h), frac = h - lo (q = 1: lo = N - 1,
        frac = 0) -> (lo [Q] ints, frac [Q] floats), what mmdyn_ensemble_quantiles is handed."""
        h = [float(q) * (N - 1) for q in quantiles]
        lo = [min(int(math.floor(x)), N - 1) for x in h]
        return lo, [x - l for x, l in zip(h, lo)]

    def _rollout_ensemble(self, T, N, per_step_cond, visual, tactile, pose, cond, avail, ov, ot, op, oav, tv, tt, tp, tav,
                          quantiles=None):
        """N sampled trajectories per request row, sample-major (row n * B + b).  Step 0 has the structure of :meth:`_iw_score`: the
        encoders, the heads and the PoE launch ONCE on the B rows (z not requested), one [N][B][L] draw, one iw_latent launch, the
        decoders on the N * B rows; every later step is the joint forward of the N * B state rows with one [N * B][L] draw.  ONE
        ensemble_feed launch closes a step: the N * B next states under the step's B observations, and the per-element mean and
        variance of the prediction over n plus each row's summed variance, from the same read of the decoder outputs.  With
        targets, the row kernels run with G = N passes against the one target (slots 0..N-1 of [N][B] tables, ops.ROW_GROUPS_MAX
        passes per launch) and the assembly of :meth:`_score_tail` on the N * B rows; tables [T][3][2][N][B], cleared by one
        fill, like ``spread``.  With ``quantiles`` (a tuple of Q numbers in [0, 1]) ONE ensemble_quantiles launch follows each
        step's feed: the Q order statistics per element of the same decoder outputs (the prediction, observed or not) and, with
        targets, of the step's ``rows`` column, as a fourth group."""
        feed, iw_latent = ops.backend_op("ensemble_feed"), ops.backend_op("iw_latent")
        (B, dev), L, S = self._rows_of(visual, tactile, pose, avail), self.L, self.model.visual_decoder.image_size
        NB = N * B
        traj = [torch.empty(T, N, B, 3, S, S, device=dev), torch.empty(T, N, B, 3, S, S, device=dev),
                torch.empty(T, N, B, 7, device=dev) if self.use_pose else None]
        shapes = ((T, B, 3, S, S), (T, B, 3, S, S)) + (((T, B, 7),) if self.use_pose else ())
        mean = [torch.empty(s, device=dev) for s in shapes] + ([] if self.use_pose else [None])
        var = [torch.empty(s, device=dev) for s in shapes] + ([] if self.use_pose else [None])
        spread = torch.zeros(T, 3, B, dtype=torch.float64, device=dev)
        means, log_var = torch.empty(T, N, B, L, device=dev), torch.empty(T, N, B, L, device=dev)
        scoring = any(t is not None for t in (tv, tt, tp))
        if scoring:
            tab = torch.zeros(T, 3, 2, N, B, dtype=torch.float64, device=dev)
            rows = torch.empty(T, N, B, device=dev)
        if quantiles is not None:
            quant, Q = ops.backend_op("ensemble_quantiles"), len(quantiles)
            q_lo, q_frac = self._quantile_index(quantiles, N)
            qs = [torch.empty((T, Q) + s[1:], device=dev) for s in shapes] + ([] if self.use_pose else [None])
            rows_q = torch.empty(T, Q, B, device=dev) if scoring else None
        state = [visual, tactile, pose]
        step_of = lambda t, i: None if t is None else t[i]
        rep = lambda t: None if t is None else t.repeat((N,) + (1,) * (t.dim() - 1))      # [B, ...] -> [N * B, ...], sample-major
        with self._index_scope():
            for i in range(T):
                c_i = step_of(cond, i) if per_step_cond else cond
                c_rows = rep(c_i)
                if i == 0:
                    mu, lv, _ = self._poe(self._heads(state[0], state[1], state[2], c_i), avail, None, B, dev)
                    eps = self._draw_latent(NB).view(N, B, L)
                    z, ratio = torch.empty(N, B, L, device=dev), torch.empty(N, B, dtype=torch.float64, device=dev)
                    iw_latent(mu, lv, eps, z, ratio, N, B, L)
                    means[0].copy_(mu)                       # the request's posterior in all N slots
                    log_var[0].copy_(lv)
                    z = z.view(NB, L)
                else:
                    mu, lv, z = self._poe(self._heads(state[0], state[1], state[2], c_rows), None, self._draw_latent(NB), NB, dev,
                                          out=(means[i].view(NB, L), log_var[i].view(NB, L)))
                v, t, pr = self._decode(z, c_rows)
                if scoring:         # before the correction below: what each trajectory predicted for frame i + 1
                    self._ensemble_tail(N, B, v, t, pr, mu, lv, step_of(tv, i), step_of(tt, i), step_of(tp, i), rep(step_of(tav, i)),
                                        tab[i], rows[i])
                flat = lambda x: x.view((NB,) + tuple(x.shape[2:]))
                groups = [{"recon": v, "obs": step_of(ov, i), "out": flat(traj[0][i]), "mean": mean[0][i], "var": var[0][i],
                           "spread": spread[i, 0], "logits": True, "column": 0},
                          {"recon": t, "obs": step_of(ot, i), "out": flat(traj[1][i]), "mean": mean[1][i], "var": var[1][i],
                           "spread": spread[i, 1], "logits": True, "column": 1}]
                if self.use_pose:
                    groups.append({"recon": pr, "obs": step_of(op, i), "out": flat(traj[2][i]), "mean": mean[2][i], "var": var[2][i],
                                   "spread": spread[i, 2], "logits": False, "column": 2})
                feed(groups, step_of(oav, i), N, B)
                if quantiles is not None:
                    qg = [{"src": g["recon"], "out": qs[m][i], "logits": g["logits"]} for m, g in enumerate(groups)]
                    if scoring:
                        qg.append({"src": rows[i].view(NB), "out": rows_q[i], "logits": False})
                    quant(qg, q_lo, q_frac, N, B)
                state = [g["out"] for g in groups] + ([] if self.use_pose else [None])
        res = {"visual": traj[0], "tactile": traj[1], "pose": traj[2], "visual_mean": mean[0], "visual_var": var[0],
               "tactile_mean": mean[1], "tactile_var": var[1], "pose_mean": mean[2], "pose_var": var[2], "spread": spread,
               "means": means, "log_var": log_var, "bce_visual": None, "bce_tactile": None, "mse_pose": None, "kl": None, "rows": None}
        if scoring:
            res.update(self._terms((tab[:, 0, 0], tab[:, 0, 1], tab[:, 1, 0]), (tv, tt, tp)), kl=tab[:, 2, 0], rows=rows)
        if quantiles is not None:
            res.update(visual_q=qs[0], tactile_q=qs[1], pose_q=qs[2], rows_q=rows_q)
        return res

    def _ensemble_tail(self, N, B, v, t, pr, mu, lv, tv, tt, tp, tavail, tab, rows):
        """The terms of one step of N * B trajectory rows into its (zeroed) fp64 tables ``tab`` [3][2][N][B] = (bce: visual,
        tactile; mse: pose, 0; kl: KL, 0) and ``rows`` [N][B]: the row kernels with G = N passes against the step's one target,
        kl_rows on the posterior that exists ([B] at step 0, its N copies made by a broadcast; [N * B] afterwards), and the
        assembly of :meth:`_score_tail` with P = 2 on the N * B rows (``tavail``: the table repeated N times, or None)."""
        NB, L = N * B, self.L
        self._row_terms(N, B, v, t, pr, tv, tt, tp, None, (tab[0, 0], tab[0, 1], tab[1, 0]))
        if mu.shape[0] == NB:
            ops.B.kl_rows(mu, lv, tab[2, 0].view(1, NB), 1, NB, L)
        else:
            kl = torch.empty(1, B, dtype=torch.float64, device=mu.device)
            ops.B.kl_rows(mu, lv, kl, 1, B, L)
            tab[2, 0].copy_(kl)
        bce, mse, kl = (tab[k].view(2, NB) for k in range(3))
        self._assemble(bce, mse, kl, rows.view(NB), tavail, NB)

    def _step_tensors(self, name, given, T, B):
        """``observed`` / ``targets`` = [visual | None, tactile | None, pose | None], each [T, B, ...] -> three contiguous fp32
        tensors / None on the engine's device; ValueError for a wrong leading (T, B), a wrong row shape, or a pose for a model
        without one."""
        if given is None:
            return [None] * 3
        if not isinstance(given, (list, tuple)) or len(given) > 3:
            raise ValueError(f"{name} must be a list [visual | None, tactile | None, pose | None]")
        given = (list(given) + [None] * 3)[:3]
        if given[2] is not None and not self.use_pose:
            raise ValueError(f"{name} holds a pose, the model has none")
        S = self.model.visual_decoder.image_size
        out = []
        for t, shape, what in zip(given, ((T, B, 3, S, S), (T, B, 3, S, S), (T, B, 7)), ("visual", "tactile", "pose")):
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shape):
                raise ValueError(f"{name}: {what} must be a tensor of shape [T={T}, B={B}, ...] = {shape}, got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            out.append(None if t is None else t.to(device=self.dev, dtype=torch.float32).contiguous())
        return out

    def _step_availability(self, name, available, T, B):
        """[T, B, 2 or 3] in the forms ``available`` takes -> the kernels' tables uint8 [T][B][4] (None stays None)."""
        if available is None:
            return None
        try:
            available = torch.as_tensor(available)
        except Exception as e:
            raise ValueError(f"{name} must be a [T, B, 2] or [T, B, 3] tensor: {e}")
        if available.dim() != 3 or tuple(available.shape[:2]) != (T, B):
            raise ValueError(f"{name} {tuple(available.shape)} is not [T={T}, B={B}, 2 or 3]")
        return self._availability(available.reshape(T * B, available.shape[2]), T * B).view(T, B, -1)

    @torch.no_grad()
    def rollout(self, x, pose=None, steps=1, available=None, condition=None, sample=False, observed=None, observed_available=None,
                targets=None, target_available=None, kl_weight=1.0, pose_multiplier=1000.0, samples=None, quantiles=None):
        """The one-step dynamics model applied to its own output ``steps`` = T times, as ONE captured graph.  With s_0 the request
        (``x``, ``pose``, ``available`` as in :meth:`forward`), for t = 0 .. T-1: the eval-mode forward of s_t (step 0 on the
        request's subset / availability table, later steps on every modality); the prediction p_{t+1} = (sigmoid(visual logits),
        sigmoid(tactile logits), pose decoder output); s_{t+1}[m][b] = ``observed[m][t][b]`` where ``observed_available[t][b][m]``
        is set, p_{t+1}[m][b] otherwise (filtering: a row that takes an observed modality keeps the predicted frames of its
        others).  One launch per step writes s_{t+1} into its slot of the returned trajectory, and the next step's encoders read
        that slot.

        ``sample=False`` decodes every step's posterior mean; ``sample=True`` draws a fresh [B, L] per step from the engine's
        Philox stream.  ``condition``: as in :meth:`forward`, held for all steps, or one per step ([T, B, condition_dim];
        categorical: indices [T, B]); :meth:`bad_condition` covers the whole call.  ``observed`` = [visual | None, tactile | None,
        pose | None], each [T, B, ...]; ``observed_available``: [T, B, 2 or 3] in the forms ``available`` takes (None: every
        given modality in every row and step; with [.., 2] the pose is observed wherever a pose tensor is given).  Default:
        nothing observed (open loop).  ``targets``: the layout of ``observed``; the terms of step t are those of :meth:`score` on
        the logits, pose output and posterior of step t against ``targets[m][t]``, before step t's observation is taken -- a fully
        observed rollout scores one-step-ahead error, an open-loop one open-loop error.  ``target_available``: as
        ``observed_available``, default all present; a (step, row, term) without a target is 0 and left out of ``rows``.

        Returns a dict of the graph's static outputs (copy what must survive the next call of the same shapes): ``visual`` /
        ``tactile`` [T, B, 3, S, S] in [0, 1] and ``pose`` [T, B, 7] (None without a pose model), slot t = s_{t+1}, observed rows
        bit for bit; ``means`` / ``log_var`` [T, B, L]; and, None without targets, ``bce_visual`` / ``bce_tactile`` / ``mse_pose``
        / ``kl`` (fp64 [T, B]; each step's own KL) and ``rows`` (fp32 [T, B]) = bce_visual + bce_tactile + pose_multiplier *
        mse_pose + kl_weight * kl.  The KL weight is read from device memory: one graph serves every weight.  Nothing
        synchronises.  ValueError: ``steps`` no integer >= 1, a wrong leading (T, B), ``observed_available`` without ``observed``
        (``target_available`` without ``targets``), a pose for a model without one, a trajectory tensor of 2^31 elements or more.

        ``samples`` (None: everything above, launch for launch): an int N >= 1, with ``sample=True``, asks for an ENSEMBLE of N
        sampled trajectories per request row and its statistics.  Step 0 runs the encoders once on the B rows and draws N latents
        of the one posterior (the structure of ``score(samples=)``); the decoders and every later step run on the N * B
        trajectory rows, sample-major, with one fresh [N * B, L] draw per step; an observation is taken by all N trajectories of
        its row; a condition and ``target_available`` are repeated N times.  One launch per step writes the N * B next states and,
        from the same read of the decoder outputs, the mean and the population variance over n of the PREDICTION p_{t+1} -- for
        every row, observed or not: under filtering, the spread before the observation is taken is the signal.  The dict then
        holds ``visual`` / ``tactile`` [T, N, B, 3, S, S] and ``pose`` [T, N, B, 7]; ``visual_mean`` / ``visual_var`` /
        ``tactile_mean`` / ``tactile_var`` [T, B, 3, S, S] and ``pose_mean`` / ``pose_var`` [T, B, 7] (None without a pose model);
        ``spread`` fp64 [T, 3, B] = the variance summed over each row's elements, per step and modality (the pose row 0 without a
        pose model; accumulated by atomics: equal to rounding between runs); ``means`` / ``log_var`` [T, N, B, L] (step 0: the
        request's posterior in all N slots); with targets ``bce_visual`` / ``bce_tactile`` / ``mse_pose`` / ``kl`` fp64 [T, N, B]
        and ``rows`` fp32 [T, N, B], each trajectory against the one target.  The graph key carries N.  ValueError: N no integer
        >= 1, ``sample=False`` (N identical trajectories), or N past what 32-bit element offsets allow.

        ``quantiles`` (with ``samples``; None: everything above, launch for launch): a sequence of 1 to 8 numbers q in [0, 1], in
        any order, duplicates allowed, asks for the prediction BAND of the ensemble: per element, the ``linear`` quantile of numpy /
        ``torch.quantile`` over the N samples of the PREDICTION p_{t+1} -- for every row, observed or not, as the mean and the
        variance.  With h = q (N - 1), lo = floor(h), frac = h - lo (formed here in fp64) and s the N values in ascending order:
        s[lo] where frac == 0, fp32(s[lo] + frac * (s[lo + 1] - s[lo])) otherwise, each fp64 operation rounded on its own; a NaN
        sample makes the quantiles of its element NaN.  One launch per step, directly after the step's feed, in the same graph.
        The dict then also holds ``visual_q`` / ``tactile_q`` [T, Q, B, 3, S, S], ``pose_q`` [T, Q, B, 7] (None without a pose
        model) and, with targets, ``rows_q`` fp32 [T, Q, B] = the quantiles over the N trajectories of ``rows`` (None without
        targets).  The graph key carries the q values.  ValueError: ``quantiles`` without ``samples``, an empty sequence or more
        than 8 entries, a q outside [0, 1] or NaN, ``samples`` > MMDYN_QUANTILE_N_MAX = 128."""
        T, sample = self._count("steps", steps, "model applications"), bool(sample)
        if samples is not None:
            samples = self._count("samples", samples, "trajectories per row")
            if not sample:
                raise ValueError("samples needs sample=True: the posterior-mean rollout would give N identical trajectories")
        if quantiles is not None:
            if samples is None:
                raise ValueError("quantiles needs samples=N: they are taken over the N trajectories of an ensemble")
            if isinstance(quantiles, (str, bytes)) or not hasattr(quantiles, "__len__") or not hasattr(quantiles, "__iter__") or \
                    torch.is_tensor(quantiles) or not 1 <= len(quantiles) <= ops.QUANTILES_MAX:
                raise ValueError(f"quantiles must be a sequence of 1 to {ops.QUANTILES_MAX} numbers in [0, 1], got {quantiles!r}")
            for q in quantiles:
                if isinstance(q, bool) or not isinstance(q, numbers.Real) or not 0.0 <= float(q) <= 1.0:
                    raise ValueError(f"quantiles must be a sequence of 1 to {ops.QUANTILES_MAX} numbers in [0, 1], got {q!r} in it")
            quantiles = tuple(float(q) for q in quantiles)
            if samples > ops.QUANTILE_N_MAX:
                raise ValueError(f"samples = {samples} is more than the quantiles rank per element (MMDYN_QUANTILE_N_MAX = "
                                 f"{ops.QUANTILE_N_MAX})")
        ins, B = self._request("rollout", x, pose, available, cast=True)
        S = self.model.visual_decoder.image_size
        self._fits("steps", T, "", B, 3 * S * S, "trajectory tensor", "steps")
        if samples is not None:
            # 32-bit element offsets: the trajectory tensors [T][N][B][3][S][S] and the decoders' largest activation [N * B] rows
            most = min(((1 << 31) - 1) // (T * B * 3 * S * S), ((1 << 31) - 1) // (B * self._decoder_row()))
            if samples > most:
                raise ValueError(f"samples = {samples} trajectories of B = {B} rows over steps = {T} make a tensor of 2^31 elements or "
                                 f"more; the largest samples for B = {B} and steps = {T} is {most}")
        per_step_cond = False
        if self.conditional and torch.is_tensor(condition):
            per_step_cond = condition.dim() == 3 or (self.categorical and condition.dim() == 2 and tuple(condition.shape) != (B, 1))
        if per_step_cond:
            if tuple(condition.shape[:2]) != (T, B):
                raise ValueError(f"a per-step condition is [T={T}, B={B}, ...], got {tuple(condition.shape)}")
            cond = self._condition(condition.reshape((T * B,) + tuple(condition.shape[2:])), T * B)
            cond = cond.view((T, B) + tuple(cond.shape[1:]))
        else:
            cond = self._condition(condition, B)
        if observed is None and observed_available is not None:
            raise ValueError("observed_available was given without observed")
        if targets is None and target_available is not None:
            raise ValueError("target_available was given without targets")
        obs = self._step_tensors("observed", observed, T, B)
        oav = self._step_availability("observed_available", observed_available, T, B)
        tg = self._step_tensors("targets", targets, T, B)
        tav = self._step_availability("target_available", target_available, T, B)
        self._set_weights(kl_weight, pose_multiplier)
        avail = self._availability(available, B)
        args = ins + [cond, avail] + obs + [oav] + tg + [tav]
        key = ("rollout", T, sample, self._pose_multiplier, per_step_cond, self._cond_key(cond)) + self._shapes(args, dtype=True)
        if samples is not None:
            key += (("samples", samples),)
            if quantiles is not None:
                key += (("quantiles", quantiles),)
            return self._run(key, lambda *a: self._rollout_ensemble(T, samples, per_step_cond, *a, quantiles=quantiles), args)
        return self._run(key, lambda *a: self._rollout(T, sample, per_step_cond, *a), args)

    @torch.no_grad()
    def inference(self, n=1, c=None):
        """``MVAE.inference(n, c)`` (vae.py:167-176): z ~ N(0, I) -> (visual, tactile) logits; ``c``: the n conditions of a
        conditional model, as in :meth:`forward`."""
        cond = self._condition(c, int(n))
        return self._run(("sample", int(n), self._cond_key(cond)), lambda c_: self._sample(int(n), c_), [cond])
