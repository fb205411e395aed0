"""Problem layer: the caller of the hot path, restated for synthetic / in-memory batches.

Mirrors the parts of /root/reference/mmdyn/pytorch/problems/problems.py that drive the model:
``Problem`` (ctor flags, ``set_optimizer`` :130-138, ``_train_epoch`` step body :148-156,
``_test_epoch`` :173-191, ``train`` :193-210, ``_anneal_KL`` :212-216), ``Reconstruction``
(``set_model`` :367-389, ``_elbo_loss`` :401-419, ``_mvae_elbo_loss`` :421-458, ``_evaluate_mvae``
:473-546, each with the per-sample ``reduce=False`` branch, best-validation checkpoint :580-586), ``SeqModeling`` (``parse_input`` :634-673,
``_evaluate_model`` :683-716) and ``DynModeling.parse_input`` (:765-803).

Out of scope here: the PNG/json dataset reader, TensorBoard event files and pose figures (the image grids
of ``_write_images`` :588-603 are written as PNG files: ``--log-images``), ``Regression``.  Batches come from
``SyntheticVisuoTactile`` (random 64x64 visual + tactile + 7-DoF pose, the BASELINE.json workload) or from any iterable yielding the reference's ``(data_input, data_target)``
lists.

Two execution modes for cnn-mvae training:
  * ``fused=True`` (default): :class:`mmdyn_hip.engine.MVAEStep`, the restructured kernel schedule;
  * ``fused=False``: the reference's own schedule -- seven ``model(...)`` calls and ``loss.backward()``
    through the autograd Functions of :mod:`mmdyn_hip.models.functional` (drop-in semantics, including
    the decoder passes whose output is discarded).
"""
import json
import math
import os
import pickle
import struct
import time
import zlib
from collections import defaultdict
from contextlib import contextmanager
from datetime import datetime
from pathlib import Path

import torch

from .. import config, ops
from ..engine import MVAEStep
from ..models import functional as Fn
from ..models.models import setup_model


class _GlobalNormClip:
    """``max_norm`` of the fused optimisers: the gradients of all parameter tensors are clipped by their global L2 norm, the
    arithmetic of ``torch.nn.utils.clip_grad_norm_``, on the device.  One ``grad_sumsq`` per tensor that has a gradient (the first
    overwrites the sum of squares, the rest accumulate), one ``grad_clip_coef``, then the clipped step per tensor.  ``max_norm=inf``
    reports the norm and never clips; ``None`` (default) is the unclipped code path."""

    def _init_clip(self, max_norm):
        self.max_norm = None if max_norm is None else ops.check_max_norm(max_norm, "max_norm")
        self._clip = self._partials = None

    def _measure(self):
        """Sum of squares, norm and coefficient of this step's gradients; returns the parameters that have one."""
        live = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if not live:
            return live
        dev = live[0].device
        need = max(ops.B.grad_sumsq_blocks(p.numel()) for p in live)
        if self._clip is None:
            self._clip = torch.zeros(4, dtype=torch.float64, device=dev)
        if self._partials is None or self._partials.numel() < need:
            self._partials = torch.empty(need, dtype=torch.float64, device=dev)
        for i, p in enumerate(live):
            ops.B.grad_sumsq(p.grad.contiguous().view(-1), self._partials, self._clip, accumulate=i > 0)
        ops.B.grad_clip_coef(self._clip, 1.0, self.max_norm)
        return live

    @property
    def grad_norm(self):
        """Global L2 norm of the last step's gradients before clipping (None before the first clipped step).  Synchronises."""
        return None if self._clip is None else float(self._clip[1])

    @property
    def clipped_steps(self):
        """Steps whose gradients were scaled down so far.  Synchronises."""
        return 0 if self._clip is None else int(self._clip[3])


class _ParamEma:
    """``ema_decay`` of the fused optimisers: an exponential moving average of every parameter tensor, kept on the device.  After
    the step's per-tensor launches: one ``ema_tick``, then one ``ema_update`` per tensor (a tensor without a gradient is averaged
    too, as torch.optim.swa_utils.AveragedModel does).  The averages start as the parameters at construction.  ``None`` (default):
    off, no launch, no buffer.  ``ema_names``: the parameters' names in order, the keys of :meth:`ema_params` (default "0", "1",
    ...).  ``ema_shared``: an :class:`mmdyn_hip.engine.MVAEStep` built with ``ema_decay`` over the same parameters -- the optimiser
    then updates THAT engine's average and count (one average per model whichever path a batch takes) and keeps none of its own."""

    def _init_ema(self, ema_decay, ema_warmup, ema_names, ema_shared):
        plist = [p for group in self.param_groups for p in group["params"]]
        names = [str(i) for i in range(len(plist))] if ema_names is None else list(ema_names)
        if len(names) != len(plist):
            raise ValueError(f"ema_names holds {len(names)} names for {len(plist)} parameter tensors")
        self._ema, self._ema_state = None, None
        if ema_shared is not None:
            if getattr(ema_shared, "ema", None) is None:
                raise ValueError("ema_shared must be an engine built with ema_decay")
            missing = [k for k in names if k not in ema_shared.ema]
            if missing:
                raise ValueError(f"ema_shared keeps no average of {missing[:3]}: pass the model's parameter names as ema_names")
            self.ema_decay, self.ema_warmup = ema_shared.ema_decay, ema_shared.ema_warmup
            self._ema = [(k, p, ema_shared.ema[k]) for k, p in zip(names, plist)]
            self._ema_state = ema_shared.ema_state
            return
        self.ema_decay = None if ema_decay is None else ops.check_ema_decay(ema_decay, "ema_decay")
        self.ema_warmup = bool(ema_warmup)
        if self.ema_decay is not None and plist:
            self._ema = [(k, p, p.detach().clone()) for k, p in zip(names, plist)]
            self._ema_state = ops.new_ema_state(self.ema_decay, self.ema_warmup, plist[0].device)

    def _ema_step(self):
        if self._ema is None:
            return
        ops.B.ema_tick(self._ema_state)
        for _, p, e in self._ema:
            ops.B.ema_update(e.view(-1), p.data.view(-1), self._ema_state)

    def ema_params(self):
        """Parameter name -> its average (live tensors: they follow the steps)."""
        if self._ema is None:
            raise ValueError("this optimiser keeps no average of its parameters: build it with ema_decay")
        return {k: e for k, _, e in self._ema}

    @property
    def ema_updates(self):
        """Updates of the average so far (0 without ``ema_decay``).  Synchronises."""
        return 0 if self._ema_state is None else int(self._ema_state[0])


class FusedAdam(_GlobalNormClip, _ParamEma, torch.optim.Optimizer):
    """torch.optim.Adam(lr) semantics (betas (0.9, 0.999), eps 1e-8, no weight decay) on the mmdyn_adam_step
    kernel, one launch per parameter tensor.  Used by the un-fused (reference-schedule) mode.  ``max_norm``: see
    :class:`_GlobalNormClip` (mmdyn_adam_step_clipped).  ``ema_decay`` / ``ema_warmup``: see :class:`_ParamEma`."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None, ema_decay=None, ema_warmup=False,
                 ema_names=None, ema_shared=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._init_clip(max_norm)
        self._init_ema(ema_decay, ema_warmup, ema_names, ema_shared)

    @torch.no_grad()
    def step(self):
        self._adam_launches()
        self._ema_step()

    def _adam_launches(self):
        if self.max_norm is not None:
            self._measure()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["m"], st["v"] = torch.zeros_like(p), torch.zeros_like(p)
                    st["state"] = torch.zeros(3, dtype=torch.float64, device=p.device)
                b1, b2 = group["betas"]
                if self.max_norm is not None:
                    ops.B.adam_step_clipped(p.data.view(-1), p.grad.contiguous().view(-1), st["m"].view(-1), st["v"].view(-1),
                                            st["state"], self._clip, group["lr"], b1, b2, group["eps"], 1.0)
                    continue
                ops.B.adam_step(p.data.view(-1), p.grad.contiguous().view(-1), st["m"].view(-1), st["v"].view(-1),
                                st["state"], group["lr"], b1, b2, group["eps"], 1.0)


class FusedSGD(_GlobalNormClip, _ParamEma, torch.optim.Optimizer):
    """torch.optim.SGD(lr, momentum=0.9, weight_decay=5e-4) -- the reference's SGD option (problems.py:132-136) -- on
    the mmdyn_sgd_step kernel.  ``max_norm``: see :class:`_GlobalNormClip` (mmdyn_sgd_step_clipped; the weight decay is added
    after the clipping, as in torch).  ``ema_decay`` / ``ema_warmup``: see :class:`_ParamEma`."""

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=5e-4, max_norm=None, ema_decay=None, ema_warmup=False,
                 ema_names=None, ema_shared=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self._init_clip(max_norm)
        self._init_ema(ema_decay, ema_warmup, ema_names, ema_shared)

    @torch.no_grad()
    def step(self):
        self._sgd_launches()
        self._ema_step()

    def _sgd_launches(self):
        if self.max_norm is not None:
            self._measure()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                first = not st
                if first:
                    st["buf"] = torch.zeros_like(p)
                if self.max_norm is not None:
                    ops.B.sgd_step_clipped(p.data.view(-1), p.grad.contiguous().view(-1), st["buf"].view(-1), self._clip,
                                           group["lr"], group["momentum"], group["weight_decay"], 1.0, first)
                    continue
                ops.B.sgd_step(p.data.view(-1), p.grad.contiguous().view(-1), st["buf"].view(-1), group["lr"],
                               group["momentum"], group["weight_decay"], 1.0, first)


class SyntheticVisuoTactile:
    """Iterable of ``(data_input, data_target)`` in the reference's collated list format
    (datasets.py:395-404): [visual, tactile, pose, available_modals(, shock)] / [visual, tactile, pose, mask],
    frames of ``seq_length`` per sequence folded into the batch dimension.  Values are U[0,1) like
    ``ToTensor`` images and min-max normalised poses (datasets.py:23-31, 407-408)."""

    def __init__(self, n_batches, batchsize, seq_length=1, device="cpu", seed=1234, size=64, shock_dim=0, absent=0.0):
        """``absent`` (default 0: every frame holds both images, the table is all ones): the share of (frame, image modality) pairs
        marked missing in ``available_modals``, drawn from a generator of its own so that every other tensor stays what it was."""
        self.n_batches, self.batchsize, self.seq_length = n_batches, batchsize, seq_length
        self.device, self.seed, self.size, self.shock_dim = device, seed, size, shock_dim
        self.absent = float(absent)

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        ga = torch.Generator().manual_seed(self.seed + 1)
        n = self.batchsize * self.seq_length
        for _ in range(self.n_batches):
            def draw():
                return [torch.rand(n, 3, self.size, self.size, generator=g), torch.rand(n, 3, self.size, self.size, generator=g),
                        torch.rand(n, 7, generator=g)]
            d, t = draw(), draw()
            d.append((torch.rand(n, 2, generator=ga) >= self.absent).to(torch.float32) if self.absent > 0 else torch.ones(n, 2))
            if self.shock_dim:
                d.append(torch.rand(n, self.shock_dim, generator=g))      # the shock force (datasets.py:395-404)
            t.append(torch.ones(n, 1, self.size, self.size))
            yield [x.to(self.device) for x in d], [x.to(self.device) for x in t]


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _write_png(path, grid):
    """``grid``: uint8 CPU tensor [H][W][3] -> an 8-bit RGB PNG, non-interlaced, filter type 0 on every scanline."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    lines = torch.cat((torch.zeros(H, 1, dtype=torch.uint8), grid.reshape(H, W * 3)), 1)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
                _png_chunk(b"IDAT", zlib.compress(lines.numpy().tobytes(), 6)) + _png_chunk(b"IEND", b""))


class Problem:
    def __init__(self, problem_args, log_dir=None, load_dataset=None, train_loader=None, test_loader=None,
                 seq_length=1, fused=True):
        self._model = None
        self._optimizer = None
        self._step = None
        self._best_loss = float("inf")
        self._logger_dict = defaultdict(list)
        self.parameters = vars(problem_args) if not isinstance(problem_args, dict) else dict(problem_args)
        # --log-images K (this build): the reference's per-epoch image log (problems.py:196-206) as PNG files under plot/, on every
        # epoch with epoch % K == 0 and on the last one; 0 (default) = off: no _sample call, no plot/ directory
        k = self.parameters.get('log_images') or 0
        if isinstance(k, bool) or not isinstance(k, int) or k < 0:
            raise ValueError(f"--log-images must be an integer >= 0 (0 for off), got {k!r}")
        self._log_images, self._logging_images = k, False
        self._img_logger_dict = {}       # key -> (a tensor or a pair of tensors, they are logits): the last batch's, by reference
        self._image_grids, self._grid_host = {}, {}
        self._cross_modal = self.parameters['input_type'] == 'visuotactile'
        self._kl_weight = self.parameters['kl_weight']
        self._pose_multiplier = self.parameters['pose_multiplier']
        self._conditional = self.parameters['conditional']
        self._categorical_conditions = None
        self._condition_dim = 0
        self._seq_length = seq_length
        self._fused = fused
        self.train_loader, self.test_loader = train_loader, test_loader
        use_gpu = torch.cuda.is_available() and not self.parameters['no_cuda']
        if not use_gpu and ops.B.name == "hip":
            raise RuntimeError("mmdyn_hip needs a ROCm GPU: there is no CPU path (run the reference for --no-cuda)")
        self._device = torch.device('cuda' if use_gpu else 'cpu')
        assert (self.parameters['input_type'] in config.INPUT_TYPES), "Input type is not implemented"
        if self.train_loader is None and self.parameters.get('dataset_path'):
            self.set_dataset()
        if log_dir:
            self.load_dir(log_dir)
        else:
            self.set_dir()
        self._set_problem()

    def set_dataset(self):
        """problems.py:110-125: the on-disk dataset at --dataset-path, decoded on the GPU (utils/datasets.py)."""
        from ..utils.datasets import dataset_setup
        self._input_size = (int(self.parameters.get('image_size', 64)),) * 2      # reference: (64, 64), problems.py:111
        self._n_channels = 3
        self.dataset_dict = dataset_setup(self.parameters['dataset_path'], self.parameters['problem_type'],
                                          input_size=self._input_size, batchsize=self.parameters['batchsize'],
                                          shuffle=True, device=self._device)
        self.train_dataset, self.test_dataset = self.dataset_dict['train_dataset'], self.dataset_dict['test_dataset']
        self.train_loader, self.test_loader = self.dataset_dict['train_loader'], self.dataset_dict['test_loader']
        self._seq_length = self.dataset_dict['seq_length']
        print(len(self.train_dataset), len(self.test_dataset))

    def _set_problem(self):
        self.set_model()
        self.set_criterion()
        self.set_optimizer()

    def load_dir(self, log_dir):
        self._log_dir = log_dir
        self._checkpoint_dir = self._log_dir + '/checkpoint/'
        self._plot_dir = self._log_dir + '/plot/'            # (created by the first logged epoch of --log-images)
        for d in (self._log_dir, self._checkpoint_dir):
            Path(d).mkdir(parents=True, exist_ok=True)

    def set_dir(self):
        date = datetime.now().strftime("_%Y_%m_%d_%H_%M_%S")
        self.load_dir('./logs/' + self.parameters['save_name'] + date)

    def set_model(self):
        raise NotImplementedError

    def set_criterion(self):
        raise NotImplementedError

    def set_optimizer(self):
        assert (self.parameters['optimizer'] in config.OPTIMIZERS), "loss name not implemented in Problem"
        # --grad-clip (this build): clip every step's gradient by its global L2 norm and log the norm; 0 (default) = off, the unclipped
        # launches; inf = log the norm, never clip
        clip = self.parameters.get('grad_clip') or None
        if clip is not None:
            clip = ops.check_max_norm(clip, "--grad-clip")
        self._grad_clip = clip
        # --ema-decay (this build): an exponential moving average of the parameters, kept on the device by the step itself and
        # written into the checkpoint as 'model_ema'; 0 (default) = off.  Training and validation compute on the live weights.
        ema = self.parameters.get('ema_decay') or None
        if ema is not None:
            ema = ops.check_ema_decay(ema, "--ema-decay")
        self._ema_decay = ema
        names = [k for k, _ in self._model.named_parameters()]
        ema_kw = dict(ema_decay=ema, ema_warmup=bool(self.parameters.get('ema_warmup')), ema_names=names)
        if self.parameters['optimizer'] == 'SGD':      # reference: momentum 0.9, weight decay 5e-4 (problems.py:132-136)
            self._optimizer = FusedSGD(self._model.parameters(), lr=self.parameters['lr'], momentum=0.9, weight_decay=5e-4,
                                       max_norm=clip, **ema_kw)
            return
        # the fused step takes the dict-shaped inputs of seq / dyn modeling (with the loss mask of --mask-loss when the model has
        # no pose term, and the shock condition of --conditional); everything else (plain reconstruction, cnn-vae, regressor,
        # --mask-loss with --use-pose, which fails in the reference too: problems.py:445-447) runs the module path
        # (decided from the model that was actually built: 'cnn-mvae' with a single-modality --input-type is a plain VAE)
        from ..models.vae import MVAE
        use_engine = (self._fused and isinstance(self._model, MVAE) and self._cross_modal
                      and isinstance(self, SeqModeling)
                      and not (self.parameters.get('mask_loss') and self.parameters.get('use_pose')))
        # fp32x3 (fp32 storage and results, the GEMMs on the bf16 matrix cores through the exact three-term operand split) is the
        # fused step's default arithmetic; the module path below always computes on the native fp32 matrix cores
        precision = self.parameters.get('precision', 'fp32x3')
        if use_engine:
            self._step = MVAEStep(self._model, lr=self.parameters['lr'], pose_multiplier=self._pose_multiplier,
                                  precision=precision, exact_running_stats=bool(self.parameters.get('exact_running_stats')),
                                  max_grad_norm=clip, ema_decay=ema, ema_warmup=ema_kw['ema_warmup'])
        elif precision not in ('fp32', 'fp32x3'):
            raise ValueError("--precision %s is a mode of the fused cnn-mvae step; this configuration runs the module "
                             "path, which computes in fp32" % precision)
        # the module path's optimiser: also what a batch the fused step does not take falls back to -- with an engine it then moves
        # the engine's average with the engine's count: one average per model, whichever path a batch takes
        if self._step is not None and ema is not None:
            ema_kw['ema_shared'] = self._step
        self._optimizer = FusedAdam(self._model.parameters(), lr=self.parameters['lr'], max_norm=clip, **ema_kw)

    def ema_state_dict(self):
        """The averaged weights as a ``state_dict`` with the model's keys (--ema-decay; None when it is off): parameters from the
        average, buffers from the live model.  The engine's average when there is an engine, the optimiser's otherwise."""
        if getattr(self, '_ema_decay', None) is None:
            return None
        if self._step is not None:
            return self._step.ema_state_dict()
        avg = self._optimizer.ema_params()
        return type(self._model.state_dict())((k, avg.get(k, v)) for k, v in self._model.state_dict().items())

    @property
    def ema_updates(self):
        """Updates of the average so far, on whichever path the batches went.  Synchronises."""
        return self._step.ema_updates if self._step is not None else self._optimizer.ema_updates

    def _anneal_KL(self, epoch):
        if epoch < self.parameters['annealing_epochs']:
            self._kl_weight = (epoch + 1) / self.parameters['annealing_epochs']
        else:
            self._kl_weight = 1

    # ---- epoch loops -----------------------------------------------------------------------------
    def _train_epoch(self, epoch):
        self._model.train()
        train_loss, n = 0.0, 0
        perf = defaultdict(float)
        dev_loss = dev_acc = None        # fused path: loss and per-pass sums accumulate ON THE DEVICE, read once per epoch
        dev_n = dev_rows = 0             # (the reference's loss.item() per step, problems.py:156, would stall the replay)
        dev_perf, dev_perf_n = None, 0   # --use-availability: the per-step means over PRESENT targets, summed on the device
        # --grad-clip: the pre-clip norms are summed where the losses are (fused: on the device, read once per epoch; module path:
        # beside the step's float(loss)); the clipped steps of the epoch are the growth of the two device-side counts
        clipping = getattr(self, '_grad_clip', None) is not None
        dev_gnorm, gnorm_sum = None, 0.0
        clipped_before = getattr(self, '_clipped_seen', 0)
        try:
            n_batches = len(self.train_loader)
        except TypeError:
            n_batches = -1
        last = None                      # --log-images: the last batch as parsed, with the module path's outputs
        for batch_idx, (data_input, data_target) in enumerate(self.train_loader):
            inputs, targets = self.parse_input(data_input, data_target)
            if self._logging_images:
                last = [inputs, targets, None]
            if self._step is not None and self._fused_applicable(inputs):
                # on the GPU the step is replayed from HIP graphs (captured once per batch shape; the annealed KL weight
                # is read from device memory); the emulation has no graphs
                run = self._step.train_step_graphed if self._device.type == 'cuda' else self._step.train_step
                # Checkpoint fidelity: the LAST step of an epoch -- what the epoch's checkpoint sees -- also runs the image
                # decoders on the subset passes whose reconstruction the reference computes and discards, so their BatchNorm
                # running buffers receive the reference's 7 (3) EMA updates of that step, in pass order (eager launches:
                # the captured graphs hold the 4-pass schedule).  With momentum 0.1 those updates carry 1 - 0.9**7 = 52 %
                # of a buffer's weight; tests/test_model_emu.py measures the residual against the reference's buffers.
                # --exact-running-stats does it on every step (identical buffers, ~1.4x the step time).
                last_exact = (batch_idx == n_batches - 1 and not self._step.exact_running_stats and
                              self.parameters.get('exact_last_step', True))
                if last_exact:
                    self._step.exact_running_stats, run = True, self._step.train_step
                avail_kw = self._avail_kw(inputs)
                try:
                    loss = run(*self._fused_io(inputs, targets), self._kl_weight, loss_mask=self._fused_mask(targets),
                               condition=inputs.get('shock') if self._conditional else None,
                               **(dict(avail_kw, kl="sample") if avail_kw else {}))
                finally:
                    if last_exact:
                        self._step.exact_running_stats = False
                if dev_loss is None:
                    dev_loss, dev_acc = torch.zeros_like(loss, dtype=torch.float64), torch.zeros_like(self._step.acc)
                dev_loss += loss.detach().to(torch.float64)
                dev_n += 1
                if clipping:
                    if dev_gnorm is None:
                        dev_gnorm = torch.zeros((), dtype=torch.float64, device=loss.device)
                    dev_gnorm += self._step.clip[1]
                if avail_kw:
                    step_perf = self._fused_perf_present_dev()
                    dev_perf = step_perf if dev_perf is None else dev_perf + step_perf
                    dev_perf_n += 1
                    continue
                dev_acc += self._step.acc
                dev_rows += self._step.last['means'].shape[0]
                continue
            else:
                self._optimizer.zero_grad()
                outputs, loss = self._evaluate_model(inputs, targets)
                loss.backward()
                self._optimizer.step()
                if last is not None:
                    last[2] = outputs
            train_loss += float(loss.detach()) if torch.is_tensor(loss) else float(loss)
            if clipping:
                gnorm_sum += self._optimizer.grad_norm or 0.0
            n += 1
            for k, v in outputs.get('perf_measure', {}).items():
                perf[k] += v
        if dev_n:
            train_loss += float(dev_loss.sum())
            if dev_n > dev_perf_n:
                for k, v in self._fused_perf(dev_acc.cpu(), dev_rows / (dev_n - dev_perf_n)).items():
                    perf[k] += v          # (sums over the epoch's steps / rows per step = the sum of the per-step means)
            if dev_perf is not None:
                for k, v in self._perf_dict(dev_perf.cpu()).items():
                    perf[k] += v
            n += dev_n
        self._logger_dict['Loss/train_epoch'].append(train_loss / max(n, 1))
        self._logger_dict['KL_annealing/train_epoch'].append(self._kl_weight)
        if clipping:
            if dev_gnorm is not None:
                gnorm_sum += float(dev_gnorm)
            self._clipped_seen = (self._step.clipped_steps if self._step is not None else 0) + self._optimizer.clipped_steps
            self._logger_dict['Grad_norm/train_epoch'].append(gnorm_sum / max(n, 1))
            self._logger_dict['Grad_clipped/train_epoch'].append(self._clipped_seen - clipped_before)
        for k, v in perf.items():
            self._logger_dict['Perf_measure_train/' + k].append(v / max(n, 1))
        if last is not None:
            self._log_batch_images('train', *last)
        return dict(perf)

    def _test_epoch(self, epoch):
        self._model.train()          # sic: the reference validates in train mode (problems.py:174)
        val_loss, n = 0.0, 0
        perf = defaultdict(float)
        last = None
        with torch.no_grad():
            for batch_idx, (data_input, data_target) in enumerate(self.test_loader):
                inputs, targets = self.parse_input(data_input, data_target)
                if self._logging_images:
                    last = [inputs, targets, None]
                if self._step is not None and self._fused_applicable(inputs):
                    avail_kw = self._avail_kw(inputs)
                    loss = self._step.eval_step(*self._fused_io(inputs, targets), self._kl_weight,
                                                loss_mask=self._fused_mask(targets),
                                                condition=inputs.get('shock') if self._conditional else None,
                               **(dict(avail_kw, kl="sample") if avail_kw else {}))
                    outputs = {'perf_measure': self._fused_perf_present() if avail_kw else self._fused_perf()}
                else:
                    outputs, loss = self._evaluate_model(inputs, targets)
                    if last is not None:
                        last[2] = outputs
                val_loss += float(loss)
                n += 1
                for k, v in outputs.get('perf_measure', {}).items():
                    perf[k] += v
        self._logger_dict['Loss/validation_epoch'].append(val_loss / max(n, 1))
        for k, v in perf.items():
            self._logger_dict['Perf_measure_validation/' + k].append(v / max(n, 1))
        if last is not None:
            self._log_batch_images('validation', *last)
        if val_loss < self._best_loss:      # best-validation checkpoint, same dict keys as problems.py:580-586
            state = {'model': self._model.state_dict(), 'loss': val_loss, 'epoch': epoch}
            if getattr(self, '_ema_decay', None) is not None:
                # --ema-decay: the averaged weights beside the live ones (copied to the host: the views go on following training)
                state['model_ema'] = type(state['model'])((k, v.detach().to('cpu', copy=True))
                                                          for k, v in self.ema_state_dict().items())
                state['ema_updates'] = self.ema_updates
            torch.save(state, self._checkpoint_dir + '/epoch_' + str(epoch) + '.ckpt')
            if self._step is not None:
                # the checkpoint keeps the reference's three keys (problems.py:751-757); how the image decoders' BatchNorm
                # running buffers in 'model' were produced goes next to it
                mode = ('exact' if self._step.exact_running_stats else
                        'exact-on-last-step-of-epoch' if self.parameters.get('exact_last_step', True) else 'live-passes-only')
                with open(self._checkpoint_dir + '/bn_running_stats_mode.txt', 'w') as f:
                    f.write(mode + '\n')
            self._best_loss = val_loss
        return dict(perf)

    def train(self, save=True):
        perf = {}
        for epoch in range(self.parameters['num_epochs']):
            t0 = time.time()
            self._anneal_KL(epoch)
            k = self._log_images
            self._logging_images = k > 0 and (epoch % k == 0 or epoch == self.parameters['num_epochs'] - 1)
            self._train_epoch(epoch)
            if self.test_loader is not None:
                perf = self._test_epoch(epoch)
            if self._logging_images:
                # the reference's order (problems.py:199-206): decoded draws from the prior, then every kept tensor as a grid
                sample = self._sample(n=50)
                if sample is not None:
                    self._img_logger_dict['Samples/latent_space'] = (sample, True)
                self._write_images(epoch)
                self._logging_images = False
            row = {k: v[-1] for k, v in self._logger_dict.items() if v}
            row.update(epoch=epoch, seconds=time.time() - t0)
            with open(os.path.join(self._log_dir, 'scalars.jsonl'), 'a') as f:
                f.write(json.dumps(row) + "\n")
            print('Epoch: %d  %s' % (epoch, json.dumps(row)))
        if save:
            with open(os.path.join(self._log_dir, 'results.pkl'), 'wb') as f:
                pickle.dump(dict(self._logger_dict), f)
        return perf

    def score(self, data_input, data_target):
        """Per-sample ELBO of one batch in the loader's format: ``parse_input``, then ``_evaluate_model(..., reduce=False)`` without
        autograd -> fp32 ``[B]``, one value per sample, in whatever mode (train / eval) the model is in.  The rows are the
        reference's (problems.py:415-417, 451-456): each holds the sample's own reconstruction terms plus ``kl_weight`` times the
        KL of the WHOLE batch, summed over the subset passes, and nothing is divided by B -- so ``rows.mean()`` is not the scalar
        loss, and differences between rows of one batch are differences of reconstruction error only."""
        inputs, targets = self.parse_input(data_input, data_target)
        with torch.no_grad():
            _, rows = self._evaluate_model(inputs, targets, reduce=False)
        return rows

    # ---- --log-images: the per-epoch image log (problems.py:196-206, 561-604, 718-739) ------------------------------------------
    def _log_batch_images(self, split, inputs, targets, outputs):
        """Keep the tensors of an epoch's last batch under the reference's keys (overridden per problem; by reference: the grids
        are launched by this epoch's :meth:`_write_images`, before any step that could write the engine's buffers again -- the
        validation steps are eager and write buffers of their own; after a capturing call of the replayed step the engine's
        ``last`` holds that call's values in the buffers the replays write).
        ``outputs``: what the module path returned, None for a batch the fused step took."""

    def _recon_images(self, outputs):
        """The image logits of a batch: ``outputs['recon_x']`` of the module path, the fused step's otherwise; a cross-modal model
        gives (visual, tactile) -- the pose is left out."""
        recon = outputs['recon_x'] if outputs is not None else self._step.last['recon_x']
        return tuple(recon[:2]) if isinstance(recon, (list, tuple)) else recon

    def _grid_source(self, key, t):
        """One tensor of the image log as the kernel takes it: contiguous fp32 [n][C][H][W]."""
        t = t.detach()
        if self.parameters['model_name'] == 'mlp-vae':        # problems.py:595-596
            s = int(self.parameters.get('image_size', 64))
            # a batch row group of the MLP is the three channel rows of one frame, so batches take the reference's view; a prior
            # draw is ONE row of s * s values (the reference's view raises on the 50 of them, and would mix three draws into one
            # RGB image where it fits): the draws go out as one-channel images, whatever their number
            t = t.reshape(-1, 1 if key.startswith('Samples') else 3, s, s)
        # the inputs and targets are the loader's fp32 frames, and the image logits are fp32 in every storage mode of the fused step
        # (the 16-bit modes store the activations BETWEEN the layers in 16 bits: include/mmdyn_hip.h), so nothing is cast here
        if t.dtype != torch.float32:
            raise TypeError(f"--log-images: the image tensor {key} is {t.dtype}; the grid kernel takes fp32")
        return t.contiguous()            # (a [::seq_length] view of the loader's frames is gathered here)

    def _write_images(self, epoch, n_images=120):
        """One ``image_grid`` launch per kept key, the grids copied into reused (pinned) host buffers behind ONE synchronisation,
        then written to ``plot/<key with '/' as '_'>_epoch_<epoch>.png``.  ``nrow`` and the number of images taken per tensor
        follow problems.py:589-593."""
        kept, self._img_logger_dict = self._img_logger_dict, {}
        if not kept:
            return
        path = str(self.parameters.get('dataset_path') or '')
        l, bs = int(self._seq_length or 1), int(self.parameters['batchsize'])
        nrow = l if (l > 1 and 'sv' not in path) else max(int(math.sqrt(bs)), 1)
        if 'modeling' in self.parameters['problem_type'] and 'sv' not in path:
            take = min(bs * l, n_images)
        else:
            take = min(bs, n_images)
        image_grid = ops.backend_op("image_grid")
        host = {}
        for key, (v, logits) in kept.items():
            srcs = [self._grid_source(key, t) for t in (v if isinstance(v, (list, tuple)) else (v,))]
            grid = image_grid(srcs, take, nrow, logits)
            buf = self._grid_host.get(key)
            if buf is None or buf.shape != grid.shape:
                buf = self._grid_host[key] = torch.empty(grid.shape, dtype=torch.uint8, pin_memory=grid.is_cuda)
            buf.copy_(grid, non_blocking=True)
            host[key] = buf
        if self._device.type == 'cuda':
            torch.cuda.current_stream().synchronize()
        Path(self._plot_dir).mkdir(parents=True, exist_ok=True)
        self._image_grids = {}
        for key, buf in host.items():
            _write_png(os.path.join(self._plot_dir, '%s_epoch_%d.png' % (key.replace('/', '_'), epoch)), buf)
            self._image_grids[key] = buf.clone()

    def image_grids(self):
        """``{key: uint8 CPU tensor [Hg, Wg, 3]}``: the grids of the latest logged epoch (``{}`` before the first, or with
        --log-images off)."""
        return dict(self._image_grids)

    _rows_kl_mode = 0        # KL of the reduce=False rows: 0 the reference's (batch total in every row); train_batch may set 1

    def train_batch(self, data_input, data_target, sample_weight=None, kl="sample"):
        """One optimiser step on one batch in the loader's format with per-sample weights: ``parse_input``, then the gradient of
        L = (1/B) sum_b w_b * row_b, where row_b is the per-sample ELBO (``kl="sample"``: with the sample's own KL -- with w = 1 the
        ordinary loss; ``kl="batch"``: the reference's reduce=False row, ``(w * rows).sum() / B``).  ``sample_weight``: [B] floats
        (None: ones) -- hard-example weights from :meth:`score`, importance or class-balance weights.  The fused engine runs where
        it takes the batch, the module path otherwise.  BatchNorm statistics are those of the unweighted batch.  Returns
        ``{"loss": the weighted scalar (device tensor), "rows": fp32 [B], the unweighted per-sample losses of this batch}``."""
        if kl not in ("batch", "sample"):
            raise ValueError("kl must be 'batch' (the reference's row: the batch-total KL) or 'sample'")
        if not isinstance(self, Reconstruction):
            raise ValueError("train_batch weights the per-sample ELBO rows of the reconstruction problems")
        self._model.train()
        inputs, targets = self.parse_input(data_input, data_target)
        if self._step is not None and self._fused_applicable(inputs):
            xs, ts = self._fused_io(inputs, targets)
            B = xs[0].shape[0]
            w = torch.ones(B, device=self._device) if sample_weight is None else sample_weight
            run = self._step.train_step_graphed if self._device.type == 'cuda' else self._step.train_step
            loss = run(xs, ts, self._kl_weight, loss_mask=self._fused_mask(targets),
                       condition=inputs.get('shock') if self._conditional else None, sample_weight=w, kl=kl)
            return {"loss": loss.detach().clone().reshape(()), "rows": self._step.last_rows["rows"].clone()}
        self._optimizer.zero_grad()
        self._rows_kl_mode = 1 if kl == "sample" else 0
        try:
            _, rows = self._evaluate_model(inputs, targets, reduce=False, _train_rows=True)
        finally:
            self._rows_kl_mode = 0
        B = rows.shape[0]
        if sample_weight is None:
            w = torch.ones(B, device=rows.device)
        else:
            if not torch.is_tensor(sample_weight) or sample_weight.numel() != B or not sample_weight.dtype.is_floating_point:
                raise ValueError(f"sample_weight must be a floating-point tensor of B = {B} values")
            w = sample_weight.detach().reshape(B).to(device=rows.device, dtype=torch.float32)
        loss = (w * rows).sum() / B
        loss.backward()
        self._optimizer.step()
        return {"loss": loss.detach(), "rows": rows.detach()}

    # ---- fused-engine plumbing -------------------------------------------------------------------
    def _fused_applicable(self, inputs):
        return isinstance(inputs, dict) and isinstance(inputs.get('model_input'), list)

    def _fused_mask(self, targets):
        return targets['loss_mask'] if self.parameters.get('mask_loss') else None

    def _fused_io(self, x, targets):
        if self.parameters['use_pose']:
            return x['model_input'] + x['input_object_pose'], targets['target_output'] + targets['target_object_pose']
        return x['model_input'], targets['target_output']

    def _fused_perf(self, acc=None, B=None):
        """Mean BCE / MSE of the single-modality passes (problems.py:499-503, 534-535) from the engine's per-pass sums
        (``acc``: those sums, or their total over several steps of ``B`` rows each)."""
        st = self._step
        B = st.last['means'].shape[0] if B is None else B
        acc = st.acc.cpu() if acc is None else acc
        npx = st.last['recon_x'][0][0].numel()              # 3 * S * S (12288 for the reference's 64 x 64)
        row = 3 if st.last.get('masked') else 0            # the perf measures are unmasked sums (problems.py:495-505)
        out = {'visual': float(acc[row, 1]) / (B * npx), 'tactile': float(acc[row, 2]) / (B * npx)}
        if st.use_pose:
            out['pose'] = float(acc[1, 6]) / (B * 7)
        return out

    # ---- --use-availability: mixed-modality batches ------------------------------------------------------------------------------
    def _avail_kw(self, inputs):
        """``{available, target_available}`` of one parsed batch when --use-availability is on and the batch carries the dataset's
        per-frame table (``input_available_modals``), else ``{}``: the keywords of the fused step and of the module path."""
        if not self.parameters.get('use_availability') or not isinstance(inputs, dict) \
                or inputs.get('input_available_modals') is None:
            return {}
        has = inputs['input_available_modals']
        return {"available": has, "target_available": self._target_available(has)}

    def _target_available(self, has):
        """[B, 3] target availability of a parsed batch (overridden per problem)."""
        raise NotImplementedError

    def _perf_dict(self, means):
        out = {'visual': float(means[0]), 'tactile': float(means[1])}
        if self.parameters['use_pose']:
            out['pose'] = float(means[2])
        return out

    def _fused_perf_present_dev(self):
        """The performance measures of the latest fused step on a mixed batch as a device tensor (fp64 [3]: visual, tactile, pose):
        the single-modality passes' term sums over the rows whose TARGET is present, divided by that many rows (and the elements of
        one) -- from the sums and counts the step's loss assembly leaves in ``last_rows``; nothing is read back here."""
        st = self._step
        lr = st.last_rows
        npx = st.last['recon_x'][0][0].numel()
        if st.last.get('masked'):        # the perf measures are unmasked sums (problems.py:495-505)
            sums = torch.stack([lr['unmasked_bce_v_rows'][1].sum(), lr['unmasked_bce_t_rows'][2].sum(), lr['term_sums'][2, 0] * 0])
        else:
            sums = torch.stack([lr['term_sums'][0, 1], lr['term_sums'][1, 2], lr['term_sums'][2, 6] if st.use_pose else
                                lr['term_sums'][2, 0] * 0])
        per = torch.tensor([npx, npx, 7], dtype=torch.float64, device=sums.device)
        return sums / (lr['present'].clamp(min=1.0) * per)

    def _fused_perf_present(self):
        return self._perf_dict(self._fused_perf_present_dev().cpu())

    @property
    def log_dir(self):
        return self._log_dir

    @property
    def model(self):
        return self._model

    @property
    def checkpoint_dir(self):
        return self._checkpoint_dir

    @property
    def plot_dir(self):
        return self._plot_dir

    @property
    def num_epochs(self):
        return self.parameters['num_epochs']

    @property
    def input_type(self):
        return self.parameters['input_type']

    @property
    def condition_dim(self):
        return self._condition_dim


class Regression(Problem):
    """Baseline regressing the object pose from one image modality (problems.py:263-359).  The reference's
    ``set_model`` passes a ``condition_dim`` keyword its Regressor does not take (problems.py:275 vs
    models.py:30) and so cannot run as shipped; here the shock dimension goes in as ``num_classes``, the
    argument the Regressor actually sizes its conditional input with (models.py:37)."""

    def set_model(self):
        self._categorical_conditions = False
        self._condition_dim = int(getattr(self.train_loader, 'shock_dim', 0) or 0)
        if self._conditional and not self._condition_dim:
            raise ValueError("--conditional needs a dataset that carries the shock force (data[4])")
        self._model = setup_model(self.parameters['model_name'], out_dim=7, conditional=self._conditional,
                                  num_classes=self._condition_dim)
        self._model.to(self._device)

    def set_criterion(self):
        self._criterion = None                # MSELoss(reduction='sum') == Fn.MSESumFn

    def parse_input(self, data, target):
        """problems.py:290-316: one image modality in, the target pose (target[2]) out, every l-th frame."""
        l, dev = self._seq_length, self._device
        if not isinstance(data, list):
            mi, to = data.to(dev), target.to(dev)
        elif len(data) == 1:
            mi, to = data[0].to(dev), target[0].to(dev)
        else:
            i = {'visual': 0, 'tactile': 1}[self.parameters['input_type']]
            mi, to = data[i][::l].to(dev), target[2][::l].to(dev)
        shock = data[4][::l].to(dev) if isinstance(data, list) and len(data) > 4 else None
        return {'model_input': mi, 'shock': shock}, to

    def _evaluate_model(self, inputs, targets, **kwargs):
        out = self._model(inputs['model_input'], inputs['shock']) if self._conditional \
            else self._model(inputs['model_input'])
        out = out.view(targets.size())
        loss = Fn.MSESumFn.apply(out, targets.contiguous())
        return {'outputs': out, 'perf_measure': {'pose': float(loss.detach()) / targets.numel()}}, loss

    def _sample(self, n=50):
        pass


class Reconstruction(Problem):

    def set_model(self):
        self._set_condition_dim()
        model_kwargs = {'condition_dim': self._condition_dim, 'input_dim': int(self.parameters.get('image_size', 64)) ** 2,
                        'architecture': self.parameters['model_name'].split('-')[0],
                        'conditional': self._conditional, 'categorical_conditions': self._categorical_conditions,
                        'latent_size': self.parameters.get('latent_size', 256)}
        if 'mvae' in self.parameters['model_name']:
            model_kwargs['use_pose'] = self.parameters['use_pose']
        self._model = setup_model(self.parameters['model_name'], cross_modal=self._cross_modal, **model_kwargs)
        self._model.to(self._device)

    def _set_condition_dim(self):
        """--conditional on a labelled dataset: the class labels are the conditions, one-hot over max(targets) + 1 classes
        (problems.py:391-393).  Without labels (or without --conditional) there is nothing to condition on."""
        dataset = getattr(self, 'train_dataset', None) or getattr(self.train_loader, 'dataset', None)
        targets = getattr(dataset, 'targets', None)
        if self._conditional and targets is not None:
            self._categorical_conditions = True
            self._condition_dim = int(torch.as_tensor(targets).max()) + 1
        else:
            self._categorical_conditions = False
            self._condition_dim = 0

    def set_criterion(self):
        self._criterion = self._mvae_elbo_loss if 'mvae' in self.parameters['model_name'] else self._elbo_loss

    @staticmethod
    def _check_reduce(reduce, reduction):
        """torch's legacy ``reduce`` flag: False turns ``reduction`` into 'none' whatever it says -- the per-sample branch."""
        if reduce:
            raise NotImplementedError("mmdyn_hip: reduce=True (the legacy spelling of reduction='sum' without the division by B) "
                                      "is not built; use reduce=None for the scalar loss or reduce=False for the per-sample one")
        if reduce is None and reduction != 'sum':
            raise NotImplementedError("mmdyn_hip: reduction=%r with reduce=None is not built (reduce=None, reduction='sum' is the "
                                      "scalar loss; reduce=False the per-sample one)" % (reduction,))

    def _elbo_loss(self, recon_x, x, means, log_var, loss_mask=None, reduce=None, reduction='sum'):
        """(BCE_sum + kl_weight * KL) / B for VAE / CVAE (problems.py:401-419).  ``reduce=False``: the reference's per-sample
        branch (:415-417), a fp32 ``[B]`` tensor ``sum(BCE, (1, 2, 3)) + kl_weight * KL`` where KL is the total over the batch
        (not divided by B).  The rows are an ordinary autograd tensor, as in the reference: ``rows.backward(w)`` and
        ``(w * rows).sum().backward()`` give the gradients of the weighted loss (the seed kernels with a per-sample scale); under
        ``torch.no_grad()`` the result carries no graph.  On a backend without the weighted seed ops the forward is unchanged and
        the backward raises ``RuntimeError`` (``ops.backend_op``): there is no fallback."""
        self._check_reduce(reduce, reduction)
        if reduce is not None:
            rows = Fn.BCERowsFn.apply(recon_x.view(x.size()), x, loss_mask)
            return Fn.ElboRowsFn.apply(rows, None, means, log_var, self._kl_weight, self._pose_multiplier, self._rows_kl_mode)
        batch_size = x.size(0)
        KLD = Fn.KLFn.apply(means, log_var)
        BCE = Fn.BCEWithLogitsSumFn.apply(recon_x.view(x.size()), x, loss_mask)
        return (BCE + self._kl_weight * KLD) / batch_size

    def _mvae_elbo_loss(self, recon_x, x, means, log_var, loss_mask=None, reduce=None, reduction='sum'):
        """Sum over modalities of BCE (images) / pose_multiplier * MSE (pose) + kl_weight * KL, over B
        (problems.py:421-458).  ``reduce=False``: the reference's per-sample branch (:451-456), a fp32 ``[B]`` tensor of the
        reconstruction terms of each sample plus ``kl_weight`` times the KL of the WHOLE batch, nothing divided by B.  An ordinary
        autograd tensor, as in the reference (see :meth:`_elbo_loss`); no graph under ``torch.no_grad()``."""
        self._check_reduce(reduce, reduction)
        assert len(recon_x) == len(x)
        if reduce is not None:
            bce = mse = None
            for i in range(len(recon_x)):
                if len(recon_x[i].size()) > 2:
                    r = Fn.BCERowsFn.apply(recon_x[i].view(x[i].size()), x[i], loss_mask)
                    bce = r if bce is None else bce + r
                else:
                    if loss_mask is not None:
                        raise ValueError("loss_mask is image-shaped and cannot multiply the (B, 7) pose term "
                                         "(the reference raises here too: problems.py:445-447)")
                    r = Fn.MSERowsFn.apply(recon_x[i], x[i])
                    mse = r if mse is None else mse + r
            return Fn.ElboRowsFn.apply(bce, mse, means, log_var, self._kl_weight, self._pose_multiplier, self._rows_kl_mode)
        batch_size = x[0].size(0)
        recon_error = 0
        kl_divergence = Fn.KLFn.apply(means, log_var)
        for i in range(len(recon_x)):
            if len(recon_x[i].size()) > 2:
                e = Fn.BCEWithLogitsSumFn.apply(recon_x[i].view(x[i].size()), x[i], loss_mask)
            else:
                if loss_mask is not None:
                    raise ValueError("loss_mask is image-shaped and cannot multiply the (B, 7) pose term "
                                     "(the reference raises here too: problems.py:445-447)")
                e = self._pose_multiplier * Fn.MSESumFn.apply(recon_x[i], x[i])
            recon_error = recon_error + e
        return (recon_error + self._kl_weight * kl_divergence) / batch_size

    def _evaluate_model(self, x, targets, reduce=None, reduction='sum', **kwargs):
        if 'mvae' in self.parameters['model_name']:
            return self._evaluate_mvae(x=x, targets=x, reduce=reduce, reduction=reduction)
        if self._conditional:
            # targets here is really the conditions (class labels): problems.py:463-465
            recon_x, means, log_var = self._model(x, targets)
        else:
            recon_x, means, log_var = self._model(x)
        loss = self._criterion(recon_x, x, means, log_var, reduce=reduce, reduction=reduction)
        return {'recon_x': recon_x, 'means': means, 'log_var': log_var}, loss

    def _evaluate_mvae_avail(self, x, targets, loss_mask, condition, available, target_available):
        """The subset schedule on a mixed-modality batch, the semantics of ``MVAEStep.forward(available=, target_available=)``:
        ``MVAE.forward(available=)`` per subset, the differentiable row functions, and a ``torch.where`` on the target table --
        L = (1/B) sum_s [ sum_b sum_{m in s, target present} rec_m(s, b) + kl_weight KL(s) ].  The performance measures are means
        over present targets."""
        m, dev = self._model, x[0].device
        B = x[0].shape[0]
        tgt = Fn.availability_table(available if target_available is None else target_available, B, dev) != 0
        use_pose = bool(self.parameters['use_pose'])
        zero = torch.zeros(B, dtype=torch.float64, device=dev)
        order = [(1, 1, 0), (1, 0, 0), (0, 1, 0)] + ([(1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1)] if use_pose else [])
        loss, perf, joint = 0, {}, None
        for a, b, c in order:
            out = m([x[0] if a else None, x[1] if b else None], pose=x[2] if c else None, condition=condition, available=available)
            means, log_var = out[3], out[4]
            rec = 0
            for on, r, col, key in ((a, out[0], 0, 'visual'), (b, out[1], 1, 'tactile')):
                if on:
                    rows = Fn.BCERowsFn.apply(r.view(targets[col].size()), targets[col], loss_mask)
                    rec = rec + torch.where(tgt[:, col], rows, zero).sum()
                    if a + b + c == 1:
                        with torch.no_grad():
                            plain = Fn.BCERowsFn.apply(r.view(targets[col].size()), targets[col], None)
                            perf[key] = float(torch.where(tgt[:, col], plain, zero).sum()) / \
                                (max(int(tgt[:, col].sum()), 1) * targets[col][0].numel())
            if c:
                if loss_mask is not None:
                    raise ValueError("loss_mask is image-shaped and cannot multiply the (B, 7) pose term "
                                     "(the reference raises here too: problems.py:445-447)")
                rows = Fn.MSERowsFn.apply(out[2], targets[2])
                rec = rec + self._pose_multiplier * torch.where(tgt[:, 2], rows, zero).sum()
                if a + b == 0:
                    perf['pose'] = float(torch.where(tgt[:, 2], rows.detach(), zero).sum()) / (max(int(tgt[:, 2].sum()), 1) * 7)
            loss = loss + (rec.to(torch.float32) + self._kl_weight * Fn.KLFn.apply(means, log_var)) / B
            if (a, b, c) == ((1, 1, 1) if use_pose else (1, 1, 0)):
                joint = [out[0], out[1]] + ([out[2]] if use_pose else [])
        return {'recon_x': joint, 'means': means, 'log_var': log_var, 'perf_measure': perf}, loss

    def _evaluate_mvae(self, x, targets, loss_mask=None, reduce=None, reduction='sum', condition=None, available=None,
                       target_available=None):
        """The reference's 3- or 7-subset schedule, one full model call per subset (problems.py:473-546)."""
        assert isinstance(x, list) and isinstance(targets, list)
        self._check_reduce(reduce, reduction)          # (before the first model call draws noise and moves running statistics)
        if reduce is None and (available is not None or target_available is not None):
            return self._evaluate_mvae_avail(x, targets, loss_mask, condition, available, target_available)
        kw = dict(loss_mask=loss_mask, reduce=reduce, reduction=reduction)
        m = self._model
        v_joint, t_joint, _, means, log_var = m([x[0], x[1]], condition=condition)
        loss = self._mvae_elbo_loss([v_joint, t_joint], [targets[0], targets[1]], means, log_var, **kw)
        v_only, _, _, means, log_var = m([x[0], None], condition=condition)
        loss = loss + self._mvae_elbo_loss([v_only], [targets[0]], means, log_var, **kw)
        _, t_only, _, means, log_var = m([None, x[1]], condition=condition)
        loss = loss + self._mvae_elbo_loss([t_only], [targets[1]], means, log_var, **kw)
        with torch.no_grad():
            n_img = targets[0].numel()
            perf = {'visual': float(Fn.BCEWithLogitsSumFn.apply(v_only, targets[0], None)) / n_img,
                    'tactile': float(Fn.BCEWithLogitsSumFn.apply(t_only, targets[1], None)) / n_img}
        if self.parameters['use_pose']:
            v_joint, t_joint, p_joint, means, log_var = m([x[0], x[1]], pose=x[2], condition=condition)
            loss = loss + self._mvae_elbo_loss([v_joint, t_joint, p_joint], [targets[0], targets[1], targets[2]],
                                               means, log_var, **kw)
            v_r, _, p_r, means, log_var = m([x[0], None], pose=x[2], condition=condition)
            loss = loss + self._mvae_elbo_loss([v_r, p_r], [targets[0], targets[2]], means, log_var, **kw)
            _, t_r, p_r, means, log_var = m([None, x[1]], pose=x[2], condition=condition)
            loss = loss + self._mvae_elbo_loss([t_r, p_r], [targets[1], targets[2]], means, log_var, **kw)
            _, _, p_only, means, log_var = m([None, None], pose=x[2], condition=condition)
            loss = loss + self._mvae_elbo_loss([p_only], [targets[2]], means, log_var, **kw)
            with torch.no_grad():
                perf['pose'] = float(Fn.MSESumFn.apply(p_only, targets[2])) / targets[2].numel()
            recon = [v_joint, t_joint, p_joint]
        else:
            recon = [v_joint, t_joint]
        return {'recon_x': recon, 'means': means, 'log_var': log_var, 'perf_measure': perf}, loss

    def _log_batch_images(self, split, inputs, targets, outputs):
        """problems.py:561-574: the inputs and the reconstruction logits of the batch."""
        self._img_logger_dict['Input_img/' + split] = (inputs, False)
        self._img_logger_dict['Output_img/' + split] = (self._recon_images(outputs), True)

    def _sample(self, n=50):
        """Decoded draws from the prior; a conditional model gets a random condition per draw (problems.py:550-555): a class index
        for a categorical model, uniform [0, 1) values for a real-valued one."""
        with torch.no_grad():
            if self._conditional:
                if self._categorical_conditions:
                    y = torch.randint(0, self._condition_dim, (n,)).unsqueeze(1).to(self._device)
                else:
                    y = torch.rand((n, self._condition_dim)).to(self._device)
                return self._model.inference(n=n, c=y)
            return self._model.inference(n=n)

    @contextmanager
    def _serving(self, slot, eval_mode=True):
        """The serving engine kept in the attribute ``slot``: built on first use or for a new model, its weights re-packed
        otherwise.  ``eval_mode``: the model is in ``eval()`` inside the block and goes back to the mode it was in."""
        from ..engine import MVAEInference
        was_training = self._model.training
        if eval_mode:
            self._model.eval()
        try:
            eng = getattr(self, slot, None)
            if eng is None or eng.model is not self._model:
                eng = MVAEInference(self._model)
                setattr(self, slot, eng)
            else:
                eng.refresh()
            yield eng
        finally:
            if eval_mode:
                self._model.train(was_training)

    def complete(self, x, sample=False):
        """The completed frames of a mixed-modality batch (cnn-mvae): ``x`` is the dict ``parse_input`` returns; its
        ``input_available_modals`` ([B, 2]: visual, tactile present per frame -- the dataset counts a constant image as missing)
        goes to :meth:`mmdyn_hip.engine.MVAEInference.complete` with the images, the pose when the model has one and, for a
        conditional model, ``x['shock']``.  Returns (visual, tactile, pose | None): present rows are the inputs, absent ones the
        model's reconstruction from what the row holds.  The serving engine is built on first use from the model as it stands
        (eval-mode arithmetic: running-estimate BatchNorm, no dropout) and re-packs the weights on every call."""
        if self.parameters.get('model_name') != 'cnn-mvae':
            raise ValueError(f"complete() serves cnn-mvae models, not {self.parameters.get('model_name')!r}")
        if not isinstance(x, dict) or not isinstance(x.get('model_input'), (list, tuple)) or len(x['model_input']) != 2:
            raise ValueError("complete() takes the dict parse_input returns for a visuotactile batch")
        pose = x.get('input_object_pose')
        pose = pose[0] if isinstance(pose, (list, tuple)) else pose
        with self._serving('_completer', eval_mode=False) as eng:
            out = eng.complete(list(x['model_input']), pose=pose, available=x.get('input_available_modals'),
                               condition=x.get('shock') if self._conditional else None, sample=sample)
            return tuple(None if t is None else t.clone() for t in out)

    def iw_score(self, data_input, data_target, samples=16):
        """The importance-weighted bound of one batch in the loader's format (cnn-mvae): ``parse_input``, then
        :meth:`mmdyn_hip.engine.MVAEInference.score` with ``samples`` draws per frame on the joint subset, with the problem's KL
        weight, pose multiplier and (``--mask-loss``) loss mask.  Returns ``{"rows": fp32 [B], "ess": fp32 [B]}``: a loss per frame
        that tightens towards -log p(x) as ``samples`` grows -- the number to compare checkpoints or rank frames by -- and the
        effective sample size of its weights.  Eval-mode arithmetic: the model is put in ``eval()`` for the call and goes back to
        the mode it was in; the serving engine is built on first use and re-packs the weights on every call (training changes
        them)."""
        if 'mvae' not in str(self.parameters.get('model_name')):
            raise ValueError(f"iw_score() serves the multimodal VAE (cnn-mvae), not {self.parameters.get('model_name')!r}")
        inputs, targets = self.parse_input(data_input, data_target)
        if not self._fused_applicable(inputs):
            raise ValueError("iw_score() takes a visuotactile batch in the loader's format (a list of tensors)")
        with self._serving('_iw_scorer') as eng:
            xs, ts = self._fused_io(inputs, targets)
            res = eng.score(list(xs[:2]), pose=xs[2] if len(xs) > 2 else None, targets=list(ts), loss_mask=self._fused_mask(targets),
                            kl_weight=self._kl_weight, pose_multiplier=self._pose_multiplier,
                            condition=inputs.get('shock') if self._conditional else None, samples=samples)
            return {"rows": res["rows"].clone(), "ess": res["ess"].clone()}

    def parse_input(self, data, target):
        if not isinstance(data, list):
            return data.to(self._device), target.to(self._device)
        it = self.parameters['input_type']
        if it == 'visual':
            mi = data[0].to(self._device)
        elif it == 'tactile':
            mi = data[1].to(self._device)
        else:
            mi = [data[0].to(self._device), data[1].to(self._device)]
        return mi, target.to(self._device) if torch.is_tensor(target) else target


class SeqModeling(Reconstruction):

    def _set_condition_dim(self):
        """condition_dim = the shock-force dimension of the dataset (problems.py:675-681)."""
        self._categorical_conditions = False
        self._condition_dim = int(getattr(self.train_loader, 'shock_dim', 0) or 0)
        if self._conditional and not self._condition_dim:
            raise ValueError("--conditional needs a dataset that carries the shock force (data[4])")

    def parse_input(self, data, target):
        """First frame of every sequence -> input, dataset's final frame -> target ([::l], problems.py:634-673)."""
        l = self._seq_length
        dev = self._device
        it = self.parameters['input_type']
        if not isinstance(data, list):
            return {'model_input': data.to(dev), 'shock': None}, {'target_output': target.to(dev), 'loss_mask': None}
        idx = {'visual': [0], 'tactile': [1], 'visuotactile': [0, 1]}[it]
        mi = [data[i][::l].to(dev) for i in idx]
        to = [target[i][::l].to(dev) for i in idx]
        if len(idx) == 1:
            mi, to = mi[0], to[0]
        if len(data) > 2:
            pose_in, avail = [data[2][::l].to(dev)], data[3][::l].to(dev)
            pose_t, mask = [target[2][::l].to(dev)], target[3][::l].to(dev)
            shock = data[4][::l].to(dev) if len(data) > 4 else None
        else:
            pose_in = avail = pose_t = mask = shock = None
        return ({'model_input': mi, 'input_object_pose': pose_in, 'input_available_modals': avail, 'shock': shock},
                {'target_output': to, 'target_object_pose': pose_t, 'loss_mask': mask})

    def _log_batch_images(self, split, inputs, targets, outputs):
        """problems.py:718-739: the inputs, the reconstruction logits and the targets of the batch."""
        self._img_logger_dict['Input_img/' + split] = (inputs['model_input'], False)
        self._img_logger_dict['Output_img/' + split] = (self._recon_images(outputs), True)
        self._img_logger_dict['Target_img/' + split] = (targets['target_output'], False)

    def _target_available(self, has):
        """Every target is the dataset's final frame of its sequence, which counts as present; so does the pose target."""
        return torch.ones(has.shape[0], 3, device=has.device)

    def _evaluate_model(self, x, targets, reduction='sum', reduce=None, **kwargs):
        self._check_reduce(reduce, reduction)
        loss_mask = targets['loss_mask'] if self.parameters['mask_loss'] else None
        if 'mvae' in self.parameters['model_name']:
            xs, ts = self._fused_io(x, targets)
            if reduce is False and getattr(self, '_step', None) is not None and self._fused_applicable(x) \
                    and not kwargs.get('_train_rows'):
                # the fused engine's evaluation schedule ending in the row kernels (the reference's rows: batch-total KL)
                res = self._step.score_step(xs, ts, self._kl_weight, loss_mask=loss_mask,
                                            condition=x.get('shock') if self._conditional else None, kl="batch")
                last = self._step.last
                return {'recon_x': last['recon_x'], 'means': last['means'], 'log_var': last['log_var'],
                        'perf_measure': self._fused_perf()}, res['rows']
            return self._evaluate_mvae(x=xs, targets=ts, loss_mask=loss_mask, reduce=reduce, reduction=reduction,
                                       condition=x.get('shock'), **(self._avail_kw(x) if reduce is None else {}))
        if self._conditional:
            recon_x, means, log_var = self._model(x['model_input'], x['shock'])
        else:
            recon_x, means, log_var = self._model(x['model_input'])
        loss = self._elbo_loss(recon_x, targets['target_output'], means, log_var, loss_mask=loss_mask, reduce=reduce,
                               reduction=reduction)
        with torch.no_grad():
            tgt = targets['target_output']
            measure = float(Fn.BCEWithLogitsSumFn.apply(recon_x, tgt, None)) / tgt.numel()
        return {'recon_x': recon_x, 'means': means, 'log_var': log_var,
                'perf_measure': {self.parameters['input_type']: measure}}, loss


class DynModeling(SeqModeling):

    def set_dataset(self):
        """The reader reports seq_length only when it has just compiled the tree (datasets.py:88-93 vs 167-171; with
        an existing pickle the reference gets None, and its ``l-1::l`` below raises).  The one-step predictor needs the
        real frame count, so it is read off the data in that case."""
        super().set_dataset()
        if self._seq_length is None:
            self._seq_length = self.train_dataset.frames_per_item

    def parse_input(self, data, target):
        """One-step-ahead targets on flat [B*L, ...] frames (problems.py:765-803): roll by -1, the last frame
        of each sequence takes the dataset's final target (images only; the pose target keeps the plain
        roll, wrap-around included, exactly as the reference does)."""
        l = self._seq_length
        dev = self._device
        idx = {'visual': [0], 'tactile': [1], 'visuotactile': [0, 1]}[self.parameters['input_type']]
        mi, to = [], []
        for i in idx:
            mi.append(data[i].to(dev))
            tgt = torch.roll(data[i], -1, dims=0).to(dev)
            tgt[l - 1::l] = target[i][l - 1::l].to(dev)
            to.append(tgt)
        if len(idx) == 1:
            mi, to = mi[0], to[0]
        shock = data[4].to(dev) if len(data) > 4 else None
        return ({'model_input': mi, 'input_object_pose': [data[2].to(dev)], 'input_available_modals': data[3].to(dev),
                 'shock': shock},
                {'target_output': to, 'target_object_pose': [torch.roll(data[2], -1, dims=0).to(dev)],
                 'loss_mask': target[3].to(dev)})

    def _target_available(self, has):
        """The target of frame b is frame b + 1 (the roll of :meth:`parse_input`): so is its availability; the last frame of a
        sequence takes the dataset's final target, which counts as present, and the pose target always counts."""
        l = int(self._seq_length)
        tgt = torch.roll(has.to(torch.float32), -1, dims=0)
        tgt[l - 1::l] = 1.0
        return torch.cat((tgt[:, :2], torch.ones(tgt.shape[0], 1, device=tgt.device)), 1)

    def _recorded_steps(self, data, target, T, n):
        """The recorded continuation of the n sequences of a loader batch over T steps: (``steps_of``, targets [visual, tactile,
        pose | None] each [T, n, ...], their availability [T, n, 3]).  The target of step t is frame t + 1 and, for t + 1 = l, the
        dataset's final target, counted as present; the pose target always counts."""
        l, dev = int(self._seq_length), self._device

        def steps_of(frames, last):
            """[T, n, ...]: frame t + 1 of every sequence for t + 1 < l, ``last`` [n, ...] for t + 1 = l."""
            f = frames.reshape((n, l) + tuple(frames.shape[1:]))[:, 1:T + 1].transpose(0, 1)
            return (f if T < l else torch.cat((f, last.unsqueeze(0).to(f.dtype)), 0)).to(dev)

        targets = [steps_of(data[0], target[0][l - 1::l]), steps_of(data[1], target[1][l - 1::l]),
                   steps_of(data[2], target[2][l - 1::l]) if self._model._use_pose else None]
        has = data[3].to(torch.float32)
        tavail = torch.cat((steps_of(has[:, :2], torch.ones(n, 2)), torch.ones(T, n, 1, device=dev)), 2)
        return steps_of, targets, tavail

    def rollout(self, data_input, data_target, steps=None, observe=(), sample=False, samples=None, quantiles=None):
        """The one-step predictor applied to its own output along each sequence of one loader batch (cnn-mvae; n sequences of l
        frames as flat [n*l, ...] tensors): :meth:`mmdyn_hip.engine.MVAEInference.rollout` from frame 0 of every sequence (with its
        ``data[3]`` availability) for ``steps`` <= l steps (default l), scored against the recorded sequence.  The target of step
        t is frame t + 1 (images with that frame's ``data[3]`` as target availability, pose ``data[2]``) and, for t + 1 = l, the
        dataset's final target (``target[i][l-1::l]``, ``target[2][l-1::l]`` for the pose -- not the wrap-around roll of
        :meth:`parse_input`), counted as present; the pose target always counts.  ``observe``: a tuple out of ("visual",
        "tactile", "pose") -- those modalities are fed back from the recorded frames t + 1 < l where the dataset has them (touch
        keeps arriving after vision is lost).  ``data[4]`` per frame is the per-step condition of a ``--conditional`` model.
        Eval-mode arithmetic: the model is put in ``eval()`` for the call and goes back to the mode it was in; the engine is
        built on first use and re-packs the weights on every call.  ``samples`` = N (with ``sample=True``): an ensemble of N sampled
        trajectories per sequence and its per-element mean / variance, as the engine's ``rollout(samples=N)`` returns them;
        ``quantiles`` (with ``samples``): the per-element quantiles of the ensemble's prediction and of ``rows``, likewise.
        Returns clones of the engine's dict."""
        if 'mvae' not in str(self.parameters.get('model_name')):
            raise ValueError(f"rollout() serves the multimodal VAE (cnn-mvae), not {self.parameters.get('model_name')!r}")
        if not isinstance(data_input, (list, tuple)) or len(data_input) < 4 or self.parameters.get('input_type') != 'visuotactile':
            raise ValueError("rollout() takes a visuotactile batch in the loader's format (a list of tensors)")
        names = ('visual', 'tactile', 'pose')
        observe = (observe,) if isinstance(observe, str) else tuple(observe)
        if any(o not in names for o in observe):
            raise ValueError(f"observe holds names out of {names}, got {observe!r}")
        l = int(self._seq_length)
        T = l if steps is None else steps
        if isinstance(T, bool) or not isinstance(T, int) or T < 1 or T > l:
            raise ValueError(f"steps must be an integer in [1, {l}] (the sequences hold {l} frames), got {steps!r}")
        data, target, dev = list(data_input), list(data_target), self._device
        if data[0].shape[0] % l:
            raise ValueError(f"a batch of {data[0].shape[0]} frames does not hold whole sequences of {l}")
        n = data[0].shape[0] // l
        use_pose = bool(self._model._use_pose)
        steps_of, targets, tavail = self._recorded_steps(data, target, T, n)
        has = data[3].to(torch.float32)
        observed = oavail = None
        if observe:
            # past the recorded frames (t + 1 = l) nothing is observed: a zero frame the table switches off
            observed = [steps_of(data[m], torch.zeros_like(data[m][l - 1::l])) if names[m] in observe and (m < 2 or use_pose)
                        else None for m in range(3)]
            inside = steps_of(torch.ones(n * l, 1), torch.zeros(n, 1))
            col = lambda m: (steps_of(has[:, m:m + 1], torch.zeros(n, 1)) if m < 2 else inside) if observed[m] is not None \
                else torch.zeros(T, n, 1, device=dev)
            oavail = torch.cat([col(m) for m in range(3)], 2)
        cond = None
        if self._conditional:
            if len(data) < 5:
                raise ValueError("a conditional model needs the shock force of every frame (data[4])")
            cond = data[4].reshape((n, l) + tuple(data[4].shape[1:]))[:, :T].transpose(0, 1).to(dev)
        with self._serving('_roller') as eng:
            res = eng.rollout([data[0][::l].to(dev), data[1][::l].to(dev)], pose=data[2][::l].to(dev) if use_pose else None,
                              steps=T, available=data[3][::l].to(dev), condition=cond, sample=sample, observed=observed,
                              observed_available=oavail, targets=targets, target_available=tavail, kl_weight=self._kl_weight,
                              pose_multiplier=self._pose_multiplier, **({} if samples is None else {"samples": samples}),
                              **({} if quantiles is None else {"quantiles": quantiles}))
            return {k: None if v is None else v.clone() for k, v in res.items()}

    def plan(self, data_input, data_target, candidates=None):
        """Which of N candidate shocks takes each frame of one loader batch to its recorded next frame (cnn-mvae, ``--conditional``):
        ``parse_input``, then :meth:`mmdyn_hip.engine.MVAEInference.plan` on the joint request with the batch's ``data[3]``
        availability, goal = the batch's target frames (the pose too if the model uses it) with the dataset's availability column
        as ``goal_available`` (the pose goal always counts), the problem's KL weight and pose multiplier, posterior-mean latents.
        ``candidates``: as the engine takes them.  Eval-mode arithmetic: the model is put in ``eval()`` for the call and goes back
        to the mode it was in; the engine is built on first use and re-packs the weights on every call.  Returns clones of the
        engine's dict plus ``recorded``: the batch's own shock, to compare the choice with."""
        if 'mvae' not in str(self.parameters.get('model_name')):
            raise ValueError(f"plan() serves the multimodal VAE (cnn-mvae), not {self.parameters.get('model_name')!r}")
        if not isinstance(data_input, (list, tuple)) or len(data_input) < 4 or self.parameters.get('input_type') != 'visuotactile':
            raise ValueError("plan() takes a visuotactile batch in the loader's format (a list of tensors)")
        if not self._conditional:
            raise ValueError("plan() was called on an unconditional model: candidate conditions need --conditional")
        if len(data_input) < 5:
            raise ValueError("a conditional model needs the shock force of every frame (data[4])")
        inputs, targets = self.parse_input(list(data_input), list(data_target))
        use_pose = bool(self._model._use_pose)
        has = inputs['input_available_modals']
        goal = list(targets['target_output']) + [targets['target_object_pose'][0] if use_pose else None]
        # the goal frame of row b is frame b + 1 (the roll of parse_input): so is its availability; the pose goal always counts
        l, dev = int(self._seq_length), self._device
        goal_has = torch.roll(has.to(torch.float32), -1, dims=0)
        goal_has[l - 1::l] = 1.0                                   # the dataset's final target
        goal_has = torch.cat((goal_has[:, :2], torch.ones(goal_has.shape[0], 1, device=dev)), 1)
        with self._serving('_planner') as eng:
            res = eng.plan(list(inputs['model_input']), pose=inputs['input_object_pose'][0] if use_pose else None, goal=goal,
                           candidates=candidates, kl_weight=self._kl_weight, pose_multiplier=self._pose_multiplier,
                           available=has, goal_available=goal_has)
            clone = lambda v: None if v is None else ([clone(t) for t in v] if isinstance(v, (list, tuple)) else v.clone())
            out = {k: clone(v) for k, v in res.items()}
            out["recorded"] = inputs['shock']
            return out

    def _horizon_batch(self, who, data_input, data_target, steps):
        """The request :meth:`plan_rollout` and :meth:`plan_refine` build from one loader batch: (T, the start = frame 0 of each of
        the n sequences as ``x`` / ``pose`` / ``available`` keywords, the goal frames 1 .. T [T, n, ...] with their availability,
        the recorded shock sequences [n, T, ...]); ValueError for a batch or a model the planners do not serve."""
        if 'mvae' not in str(self.parameters.get('model_name')):
            raise ValueError(f"{who}() serves the multimodal VAE (cnn-mvae), not {self.parameters.get('model_name')!r}")
        if not isinstance(data_input, (list, tuple)) or len(data_input) < 4 or self.parameters.get('input_type') != 'visuotactile':
            raise ValueError(f"{who}() takes a visuotactile batch in the loader's format (a list of tensors)")
        if not self._conditional:
            raise ValueError(f"{who}() was called on an unconditional model: candidate conditions need --conditional")
        if len(data_input) < 5:
            raise ValueError("a conditional model needs the shock force of every frame (data[4])")
        l = int(self._seq_length)
        T = l if steps is None else steps
        if isinstance(T, bool) or not isinstance(T, int) or T < 1 or T > l:
            raise ValueError(f"steps must be an integer in [1, {l}] (the sequences hold {l} frames), got {steps!r}")
        data, target, dev = list(data_input), list(data_target), self._device
        if data[0].shape[0] % l:
            raise ValueError(f"a batch of {data[0].shape[0]} frames does not hold whole sequences of {l}")
        n = data[0].shape[0] // l
        _, goal, goal_has = self._recorded_steps(data, target, T, n)
        recorded = data[4].reshape((n, l) + tuple(data[4].shape[1:]))[:, :T].to(dev)
        if recorded.dim() == 3 and self._model.categorical_conditions and recorded.shape[2] == 1:
            recorded = recorded[:, :, 0]
        start = dict(x=[data[0][::l].to(dev), data[1][::l].to(dev)], pose=data[2][::l].to(dev) if self._model._use_pose else None,
                     available=data[3][::l].to(dev))
        return T, start, goal, goal_has, recorded

    def plan_rollout(self, data_input, data_target, candidates=None, steps=None, step_weight=None, top=None):
        """Which of N candidate shock SEQUENCES takes frame 0 of each of the n sequences of one loader batch along its recorded
        continuation (cnn-mvae, ``--conditional``): :meth:`mmdyn_hip.engine.MVAEInference.plan_rollout` with the batch built as
        :meth:`rollout` builds it -- start = frame 0 of every sequence with its ``data[3]`` availability, goal = frames 1 .. T with
        their availability (the dataset's final target for t + 1 = l; the pose goal always counts), every step scored --, the
        problem's KL weight and pose multiplier, posterior-mean latents.  ``candidates``: as the engine takes them; None: the
        batch's own n recorded shock sequences (``data[4]``, [n, T, ...]), shared by every row, so the row's own sequence is
        candidate b.  ``steps`` <= l (default l), ``step_weight`` [T], ``top``: as the engine takes them.  Eval-mode arithmetic as
        in :meth:`plan`.  Returns clones of the engine's dict plus ``recorded``: the [n, T, ...] shocks."""
        T, start, goal, goal_has, recorded = self._horizon_batch('plan_rollout', data_input, data_target, steps)
        with self._serving('_horizon_planner') as eng:
            res = eng.plan_rollout(steps=T, goal=goal, candidates=recorded if candidates is None else candidates,
                                   step_weight=step_weight, top=top, kl_weight=self._kl_weight, pose_multiplier=self._pose_multiplier,
                                   goal_available=goal_has, **start)
            return self._cloned(res, recorded)

    @staticmethod
    def _cloned(res, recorded):
        """Clones of an engine's result dict (its tensors are a graph's static outputs) plus ``recorded``."""
        clone = lambda v: None if v is None else ([clone(t) for t in v] if isinstance(v, (list, tuple)) else v.clone())
        out = {k: clone(v) for k, v in res.items()}
        out["recorded"] = recorded
        return out

    def plan_refine(self, data_input, data_target, steps=None, candidates=64, elites=8, iterations=4, init_mean=None, init_std=None,
                    bounds=None, alpha=0.0, std_min=0.0, step_weight=None, sample=False, temperature=None, warm_start=None, shift=1,
                    widen=0.0):
        """The shock sequence that takes frame 0 of each of the n sequences of one loader batch along its recorded continuation,
        searched by the cross-entropy method (cnn-mvae, ``--conditional`` with real-valued shocks):
        :meth:`mmdyn_hip.engine.MVAEInference.plan_refine` on the request :meth:`plan_rollout` builds, every step scored, the
        problem's KL weight and pose multiplier.  ``init_mean`` / ``init_std`` default to the per-(step, dimension) mean and
        population standard deviation of the batch's n recorded shock sequences, ``bounds`` to their per-dimension minimum and
        maximum; ``candidates`` / ``elites`` / ``iterations`` / ``alpha`` / ``std_min`` / ``step_weight`` / ``sample`` / ``temperature`` (MPPI weights) /
        ``warm_start`` / ``shift`` / ``widen`` (the previous result, moved on: a receding horizon): as the engine takes them.  Eval-mode arithmetic as in :meth:`plan`.  Returns clones of the engine's dict plus ``recorded``."""
        T, start, goal, goal_has, recorded = self._horizon_batch('plan_refine', data_input, data_target, steps)
        if self._model.categorical_conditions:
            raise ValueError("plan_refine() refits a distribution over real-valued shocks; a categorical model is out of scope")
        shocks = recorded.to(torch.float32)
        if init_mean is None:
            init_mean = shocks.mean(0)
        if init_std is None:
            init_std = shocks.std(0, unbiased=False)
        if bounds is None:
            flat = shocks.reshape(-1, shocks.shape[-1])
            bounds = (flat.min(0).values, flat.max(0).values)
        with self._serving('_refiner') as eng:
            res = eng.plan_refine(steps=T, goal=goal, init_mean=init_mean, init_std=init_std, candidates=candidates, elites=elites,
                                  iterations=iterations, alpha=alpha, std_min=std_min, bounds=bounds, step_weight=step_weight,
                                  kl_weight=self._kl_weight, pose_multiplier=self._pose_multiplier, goal_available=goal_has,
                                  sample=sample, temperature=temperature, warm_start=warm_start, shift=shift, widen=widen, **start)
            return self._cloned(res, recorded)
