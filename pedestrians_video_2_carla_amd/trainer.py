"""Minimal trainer: the Lightning loop the reference delegates to, reduced to what the train step needs
(reference modeling.py:275-282 ``pl.Trainer.from_argparse_args(...).fit(model, datamodule)``).

Hook order per step is Lightning's: ``on_train_batch_start`` -> ``training_step`` -> backward -> optimizer step.
Two execution modes:
  * eager: every launch issued from Python;
  * ``use_graph=True``: the step (model forward, HIP pose head forward/backward, optimizer) is captured once into a
    HIP graph on STATIC batch buffers owned by the trainer and replayed. Every new batch is *staged* first -- copied
    into the static buffers (ONE launch for all tensors, p2c_copy_group) and handed to ``flow.on_train_batch_start`` (per-batch constants:
    skeleton-type index, target-pair counts) -- outside the graph; passing the same batch object again (a resident
    batch, as bench.py does) stages nothing. With more than one rank the gradient all-reduce is captured into the
    step graph when every rank can do so, otherwise it stays outside (capture A: forward + backward; eager RCCL
    all-reduce; optimizer launch).
``gradient_clip_val`` / ``gradient_clip_algorithm`` are Lightning's arguments of the same names: the clip runs inside FlatAdamW's
launches (K29, csrc/p2c_grad_clip.hip) -- after the all-reduce, so the averaged gradient is what is clipped -- or through
torch.nn.utils.clip_grad_* for any other optimizer; with a clip the optimizer is never fused into a backward.
``max_epochs`` / ``check_val_every_n_epoch`` / ``callbacks`` and ``fit(..., val_batches=, ckpt_path=)`` turn ``fit`` into the epoch
loop (``_fit_epochs``: validation -> epoch-interval LR schedulers -> callbacks at the end of every epoch); ``save_checkpoint`` /
``load_checkpoint`` (checkpoint.py) carry everything a resumed run needs to be the uninterrupted one, bit for bit. None of it
runs per step: the step's launches are the same with and without it.
"""
import contextlib
import gc
import os
import sys
import weakref
from typing import Dict, Iterable, List, Optional

import torch
import torch.distributed as dist

from pedestrians_video_2_carla_amd.parallel.flat import FlatParameters, GradientExchange


def seed_everything(seed: int = 22742):
    """``pl.seed_everything(seed, workers=True)`` (reference modeling.py:350-351; default seed :120-121)."""
    import random
    import numpy as np
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    os.environ['PL_GLOBAL_SEED'] = str(seed)


def init_distributed(backend: Optional[str] = None) -> Dict[str, int]:
    """One process per GPU, rendezvous from the torchrun env (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    forced = os.environ.get('P2C_FORCE_EXCHANGE', '0') == '1' and 'RANK' in os.environ   # one-rank rehearsal of the DP path
    if (world > 1 or forced) and not dist.is_initialized():
        if backend is None:
            backend = 'nccl' if torch.cuda.is_available() else 'gloo'      # "nccl" IS RCCL on ROCm
        if backend == 'nccl':
            torch.cuda.set_device(local_rank)
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return {'world_size': world, 'rank': rank, 'local_rank': local_rank}


def ranks_agree(ok: bool, device, checksum: Optional[torch.Tensor] = None, group=None) -> bool:
    """Eager agreement of all ranks on a local outcome: True only if EVERY rank passed ``ok`` and -- when given -- every
    rank holds the same finite ``checksum`` (a 0-dim float64 tensor). Two small all-reduces (MIN / MAX); every rank must
    call it the same number of times, whatever happened locally."""
    chk = checksum.detach().to(device=device, dtype=torch.float64).reshape(()) if (checksum is not None and ok) \
        else torch.zeros((), dtype=torch.float64, device=device)
    votes = torch.stack((torch.tensor(1.0 if ok else 0.0, dtype=torch.float64, device=device), chk))
    lo, hi = votes.clone(), votes.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
    return bool(lo[0] > 0.5) and bool(torch.isfinite(lo[1])) and bool(torch.isfinite(hi[1])) and float(hi[1]) == float(lo[1])


class Trainer:
    def __init__(self, max_steps: Optional[int] = None, use_graph: bool = False, device: Optional[torch.device] = None,
                 flatten: bool = True, log_every_n_steps: int = 0, steps_per_epoch: Optional[int] = None,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: str = 'norm',
                 loggers: Optional[Iterable] = None, max_epochs: Optional[int] = None, check_val_every_n_epoch: int = 1,
                 callbacks: Optional[Iterable] = None):
        # ``max_steps``: 100 when neither it nor ``max_epochs`` is given; with ``max_epochs`` alone the epochs bound the run, with
        # both whichever comes first (Lightning's rule)
        if max_steps is None and max_epochs is None:
            max_steps = 100
        if check_val_every_n_epoch < 1:
            raise ValueError(f'check_val_every_n_epoch must be at least 1, not {check_val_every_n_epoch!r}')
        self.max_epochs = max_epochs
        self.check_val_every_n_epoch = int(check_val_every_n_epoch)
        self.callbacks: List = list(callbacks) if callbacks is not None else []
        self.callback_metrics: Dict[str, float] = {}      # the monitors of the last validation / test epoch
        self._ref_params: List[torch.nn.Parameter] = []   # the parameters in the order the plugin gave them to its optimizer
        self._flow_ref = None                             # weak: flow.trainer points here, a cycle would leave GPU objects to the GC
        self._train_batches = None
        self._rng_after_capture = None                    # set by a full checkpoint load (checkpoint.load)
        # Lightning's names and defaults (the reference's trainer takes them from argparse, modeling.py:275, 353): None / 0 = off
        if gradient_clip_algorithm not in ('norm', 'value'):
            raise ValueError(f"gradient_clip_algorithm must be 'norm' or 'value', not {gradient_clip_algorithm!r}")
        if gradient_clip_val is not None and not (0.0 <= float(gradient_clip_val) < float('inf')):
            raise ValueError(f'gradient_clip_val must be finite and not negative, not {gradient_clip_val!r}')
        self.gradient_clip_val = float(gradient_clip_val) if gradient_clip_val else None
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.last_grad_norm: Optional[torch.Tensor] = None      # norm mode, after a step: a device scalar nothing syncs on
        self._clip_in_kernel = False
        self.max_steps = max_steps
        self.use_graph = use_graph
        self.device = device
        self.flatten = flatten
        self.log_every_n_steps = log_every_n_steps
        self.steps_per_epoch = steps_per_epoch
        self.datamodule = None
        self.loggers: List = list(loggers) if loggers is not None else []       # a PedestrianLogger in here writes clips
        self.global_step = 0
        self.current_epoch = 0
        self.flat: Optional[FlatParameters] = None
        self.exchange: Optional[GradientExchange] = None
        self.optimizers: List[torch.optim.Optimizer] = []
        self.lr_schedulers: List[dict] = []
        self._graphs = None
        self._static_loss = None
        self._static_batch = None
        self._staged_src = None
        self._group_copy = None
        self._direct = None
        self._unit = None
        self._packed = []
        self._opt_in_backward = False
        self._fused_seen = 0
        self._grad_sinks = False
        self._kept_graph = False
        self._graph_nodes = None
        self._handed_over = None

    @property
    def _flow(self):
        """The flow of the last ``setup`` (held weakly: ``flow.trainer`` is the strong direction. A trainer in a reference cycle is
        destroyed by the cyclic collector at a time of its choosing, and releasing captured graphs, events or pinned buffers while
        ANOTHER trainer's stream capture is open aborts the process)."""
        return self._flow_ref() if self._flow_ref is not None else None

    # ------------------------------------------------------------------------------------------------------------
    def setup(self, flow, datamodule):
        self.datamodule = datamodule
        flow.trainer = self
        self._flow_ref = weakref.ref(flow)
        if self.device is not None:
            flow.to(self.device)
        flow.train()
        configs = flow.configure_optimizers()
        if self.flatten:
            self.flat = FlatParameters(flow.parameters())
            self.exchange = GradientExchange(self.flat)
            self.exchange.broadcast_parameters(0)
            self.exchange.broadcast_buffers(flow, 0)      # DDP broadcasts module buffers (BatchNorm statistics) at wrap time
            extra = {}
            if self.flat.flat_param.is_cuda:
                extra['fused'] = True              # one kernel for the whole (flat) parameter
                extra['capturable'] = bool(self.use_graph)
                # plugins with a fused backward write their parameter gradients straight into the flat buffer
                for m in flow.modules():
                    if hasattr(m, 'grad_sink'):
                        m.grad_sink = True
                self._grad_sinks = True          # K12 adds weight gradients straight into the flat gradient buffer's views
            if len(configs) != 1:
                raise ValueError('exactly one trainable plugin expected (ZeroTrajectory has no optimizer)')
            self._ref_params = [p for g in configs[0]['optimizer'].param_groups for p in g['params']]   # (checkpoint layout)
            self.optimizers = [self.flat.rebuild_optimizer(configs[0]['optimizer'], **extra)]
            opt = self.optimizers[0]
            # modules with a re-laid-out copy of their weights (the fused MLP's LDS image) let the optimizer keep it current
            self._packed = [m for m in flow.modules() if hasattr(m, 'manage_packed_image')
                            and m.manage_packed_image(self.flat.flat_param, opt)]
            # single GPU: a module that owns every parameter can apply the optimizer step inside its own backward
            # (a gradient clip needs the global norm before the first parameter is touched: no module is offered the optimizer)
            self._opt_in_backward = (self.gradient_clip_val is None
                                     and not self.exchange.enabled and os.environ.get('P2C_FUSED_UPDATE', '1') == '1'
                                     and any(m.accept_fused_optimizer(opt, self.flat.flat_param) for m in self._packed
                                             if hasattr(m, 'accept_fused_optimizer')))
            self._fused_seen = getattr(opt, 'fused_steps_applied', 0)
            # K29: FlatAdamW clips inside its own launches; any other optimizer (another class, host tensors) and
            # P2C_CLIP_FRAMEWORK=1 (timing comparisons) take torch.nn.utils.clip_grad_* in _optimizer_step
            self._clip_in_kernel = (self.gradient_clip_val is not None and hasattr(opt, 'set_clip')
                                    and os.environ.get('P2C_CLIP_FRAMEWORK', '0') != '1')
            if self._clip_in_kernel:
                opt.set_clip(self.gradient_clip_val, self.gradient_clip_algorithm)
            framework_clip = self.gradient_clip_val is not None and not self._clip_in_kernel
            # FlatAdamW folds the DP averaging into its pass (the tensor-path clip needs the averaged gradient itself)
            if hasattr(opt, 'grad_scale') and self.exchange.enabled and not framework_clip:
                opt.grad_scale = 1.0 / self.exchange.world
                self.exchange.average_here = False
        else:
            self.optimizers = [c['optimizer'] for c in configs]
        # LR schedulers (base_model.py:159-199) were built on the plugin's own optimizer: re-bind them to the one that steps
        self.lr_schedulers = []
        for c, opt in zip(configs, self.optimizers):
            sched = c.get('lr_scheduler')
            if sched is None:
                continue
            sched = dict(sched) if isinstance(sched, dict) else {'scheduler': sched}
            sched.setdefault('interval', 'epoch')        # Lightning's defaults
            sched.setdefault('frequency', 1)
            s = sched['scheduler']
            if s.optimizer is not opt:
                for g_new, g_old in zip(opt.param_groups, s.optimizer.param_groups):
                    g_new.setdefault('initial_lr', g_old.get('initial_lr', g_old['lr']))
                    g_new['lr'] = g_old['lr']
                s.optimizer = opt
            self.lr_schedulers.append(sched)
        return self

    def step_lr_schedulers(self, interval: str = 'epoch', monitor: Optional[Dict[str, float]] = None):
        """What Lightning does at the end of an epoch / step for the configured schedulers. ``monitor``: logged values for
        ReduceLROnPlateau (``{'val_loss/primary': ...}``); a plateau scheduler whose key is missing is skipped, as Lightning
        would raise only in strict mode. The captured optimizer launch reads the LR from device memory
        (FlatAdamW.sync_hyper), so the change reaches graph replays."""
        count = self.current_epoch if interval == 'epoch' else self.global_step
        for sched in self.lr_schedulers:
            if sched['interval'] != interval or count % sched['frequency'] != 0:
                continue
            s = sched['scheduler']
            if isinstance(s, torch.optim.lr_scheduler.ReduceLROnPlateau):
                value = (monitor or {}).get(sched.get('monitor'))
                if value is not None:
                    s.step(value)
            else:
                s.step()

    def _zero_grad(self):
        if self.flat is not None:
            if getattr(self.optimizers[0], 'zero_grad_in_step', False):
                return                  # the flat gradient starts zeroed and FlatAdamW leaves it zeroed after each step
            self.flat.zero_grad()
        else:
            for o in self.optimizers:
                o.zero_grad(set_to_none=True)

    def _forward_backward(self, flow, batch, batch_idx, batch_start: bool = True):
        self._zero_grad()
        # forward and backward happen back to back in here and nothing reads a loss VALUE in between (the reference's
        # per-loss isnan check is off unless strict_nan_check): the pose head may leave the last stage of its loss
        # reduction to the backward kernel, or run only in the backward at all (P2C_DEFER_FINALIZE=0|1|2, see
        # ops.deferred_loss_finalize)
        mode = int(os.environ.get('P2C_DEFER_FINALIZE', '2'))      # 2: the pose head runs once per step, in the backward
        defer = batch[0].is_cuda and not getattr(flow, 'strict_nan_check', False) and mode != 0
        from pedestrians_video_2_carla_amd import ops
        with (ops.deferred_loss_finalize(mode) if defer else contextlib.nullcontext()), ops.grad_sinks(self._grad_sinks):
            if batch_start:
                flow.on_train_batch_start(batch, batch_idx)
            out = flow.training_step(batch, batch_idx)
            loss = out['loss']
            if self._unit is None or self._unit.shape != loss.shape or self._unit.device != loss.device:
                self._unit = torch.ones_like(loss)   # root gradient, made once (backward() would fill one per step)
            loss.backward(gradient=self._unit)
        return loss.detach()

    def _optimizer_step(self):
        if self._opt_in_backward:
            # normally applied by the backward launch of the module that owns the parameters -- but only if that launch
            # really ran this step (module in eval(), host tensors, detached .grad views ... take other paths)
            applied = self.optimizers[0].fused_steps_applied
            if applied != self._fused_seen:
                self._fused_seen = applied
                return
        if self.gradient_clip_val is not None and not self._clip_in_kernel:
            params = [p for o in self.optimizers for g in o.param_groups for p in g['params'] if p.grad is not None]
            if self.gradient_clip_algorithm == 'norm':
                self.last_grad_norm = torch.nn.utils.clip_grad_norm_(params, self.gradient_clip_val)
            else:
                torch.nn.utils.clip_grad_value_(params, self.gradient_clip_val)
        for o in self.optimizers:
            o.step()
        if self._clip_in_kernel:
            self.last_grad_norm = self.optimizers[0].last_grad_norm

    # ---- static batch (graph mode) -----------------------------------------------------------------------------------
    @staticmethod
    def _batch_tensors(batch):
        frames, targets, meta = batch
        out = [('frames', frames)]
        out += [('targets/' + k, v) for k, v in sorted(targets.items()) if isinstance(v, torch.Tensor)]
        out += [('meta/' + k, v) for k, v in sorted(meta.items()) if isinstance(v, torch.Tensor)]
        return out

    def _with_skel_type(self, batch):
        """meta['skel_type'] as a device tensor (data/carla/reference.py:skeleton_types_from_meta): inside a captured step
        the per-clip (age, gender) strings cannot be looked at again."""
        frames, targets, meta = batch
        st = meta.get('skel_type')
        if isinstance(st, torch.Tensor) and st.dtype == torch.int32 and st.device == frames.device:
            return batch
        # ALWAYS an int32 tensor on the frames' device, also for an int64 / host tensor and for the default adult-female
        # case without age / gender: the static batch then owns it and ProjectionModule.on_batch_start (whose `.to()` calls
        # are no-ops on it) hands the captured step that same storage for every staged batch
        from pedestrians_video_2_carla_amd.data.carla import reference as ref
        meta = dict(meta)
        meta['skel_type'] = ref.skeleton_types_from_meta(meta, batch_size=len(frames), strict=True, device=frames.device)
        return frames, targets, meta

    def stage_batch(self, flow, batch, batch_idx: int = 0):
        """Make ``batch`` the content of the static buffers the captured step reads (no-op for the batch OBJECT staged
        last: a resident batch), then run the flow's per-batch hook on them. Returns the static batch."""
        if self._static_batch is not None and batch is self._staged_src:
            return self._static_batch
        key, batch = batch, self._with_skel_type(batch)
        if self._static_batch is None:
            frames, targets, meta = batch
            clone = lambda d: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}   # noqa: E731
            self._static_batch = (frames.clone(), clone(targets), clone(meta))
            named = self._batch_tensors(self._static_batch)
            self._static_names, self._static_dst = [k for k, _ in named], [v for _, v in named]
        else:
            frames, targets, meta = batch
            try:        # the same tensors, in the order of the static list (no sorting / renaming per batch)
                src = [frames if k == 'frames' else (targets[k[8:]] if k[0] == 't' else meta[k[5:]]) for k in self._static_names]
            except KeyError as e:
                raise RuntimeError(f'graph mode needs batches of one fixed structure: {e.args[0]!r} is missing') from None
            n_tensors = 1 + sum(isinstance(v, torch.Tensor) for v in targets.values()) + sum(isinstance(v, torch.Tensor) for v in meta.values())
            if n_tensors != len(src) or any(s.shape != d.shape or s.dtype != d.dtype for s, d in zip(src, self._static_dst)):
                raise RuntimeError('graph mode needs batches of one fixed structure: got '
                                   f'{[(k, tuple(v.shape)) for k, v in self._batch_tensors(batch)]} after '
                                   f'{[(k, tuple(v.shape)) for k, v in zip(self._static_names, self._static_dst)]}')
            if self._group_copy is None and src[0].is_cuda and all(d.is_contiguous() for d in self._static_dst):
                from pedestrians_video_2_carla_amd import ops
                self._group_copy = ops.GroupCopy(self._static_dst)           # one launch for all tensors of the batch
            if self._group_copy is not None and all(t.is_cuda and t.device == d.device for t, d in zip(src, self._static_dst)):
                self._group_copy(src)
            else:
                torch._foreach_copy_(self._static_dst, src)
            for k, v in meta.items():                     # lists of strings etc. travel by reference
                if not isinstance(v, torch.Tensor):
                    self._static_batch[2][k] = v
        self._staged_src = key
        flow.on_train_batch_start(self._static_batch, batch_idx)
        return self._static_batch

    # ------------------------------------------------------------------------------------------------------------
    def train_step(self, flow, batch, batch_idx: int = 0) -> torch.Tensor:
        """One optimisation step on ``batch``; returns the (device) loss tensor."""
        if not self.use_graph:
            loss = self._forward_backward(flow, batch, batch_idx)
            if self.exchange is not None:
                self.exchange.all_reduce_gradients()
            self._optimizer_step()
        else:
            if self._direct is None or not self._hand_over(flow, batch):
                static = self.stage_batch(flow, batch, batch_idx)      # copies only when a NEW batch object arrives
            if self._graphs is None:
                # No cyclic collection while a capture is open: an object it finalises there (another trainer's graph, a loader's
                # pinned buffers and events, in a cycle the user's code made) calls the runtime from inside the capture, which aborts
                # the process. Collected before, paused during.
                gc.collect()
                gc_was_enabled = gc.isenabled()
                gc.disable()
                try:
                    self._capture(flow, static, batch_idx)
                finally:
                    if gc_was_enabled:
                        gc.enable()
                if self._rng_after_capture is not None:
                    # resumed from a checkpoint: the warm-up steps of the capture drew from the generators; the first replay
                    # must start where the uninterrupted run's next step did
                    cpu_state, cuda_state = self._rng_after_capture
                    self._rng_after_capture = None
                    if cpu_state is not None:
                        torch.set_rng_state(cpu_state)
                    if cuda_state is not None:
                        torch.cuda.set_rng_state(cuda_state, static[0].device)
                if not self.use_graph:              # the captured step failed its replay check: eager steps from here on
                    return self.train_step(flow, batch, batch_idx)
            g_fb, g_opt = self._graphs
            for o in self.optimizers:
                if hasattr(o, 'sync_hyper'):
                    o.sync_hyper()               # LR-scheduler changes reach the captured optimizer launch
            if self._direct is not None:            # the step IS one recorded call: two launches, no graph start-up
                d = self._direct
                if torch.cuda.current_device() != d['device_index']:   # the recorded pointers belong to the trainer's GPU
                    with torch.cuda.device(d['device_index']):
                        rc = d['call'](d['desc_ref'], d['gl'], torch.cuda.current_stream(d['device_index']).cuda_stream)
                else:
                    rc = d['call'](d['desc_ref'], d['gl'], torch.cuda.current_stream().cuda_stream)
                if rc != 0:
                    raise RuntimeError(f'p2c_train_step failed in direct replay (rc={rc})')
            else:
                g_fb.replay()
            if g_opt is not None:
                self.exchange.all_reduce_gradients()
                if g_opt == 'eager':
                    self._optimizer_step()
                else:
                    g_opt.replay()
            loss = self._static_loss
        self.global_step += 1
        flow.global_step = self.global_step
        if self.lr_schedulers:
            self.step_lr_schedulers('step')
        return loss

    # ---- direct replay: a new batch is handed over by ADDRESS ---------------------------------------------------------------
    def _handover_info(self, flow, static_batch):
        """What the recorded p2c_train_step call reads from a batch: (targets key of the 2-D target or None, whether the 3-D
        target is read) and the tensors' shapes -- worked out once, on the static batch the step was captured on."""
        frames, targets, meta = static_batch
        plan = flow._fused_train_plan(frames, targets) if hasattr(flow, '_fused_train_plan') else None
        st = meta.get('skel_type') if isinstance(meta, dict) else None
        if plan is None or not isinstance(st, torch.Tensor):
            return None
        _spec, gt2d, gt3d = plan
        key2 = next((k for k, v in targets.items() if v is gt2d), None) if gt2d is not None else None
        key3 = next((k for k, v in targets.items() if v is gt3d), None) if gt3d is not None else None
        if (gt2d is not None and key2 is None) or (gt3d is not None and key3 is None):
            return None
        d = self._direct['desc']
        # the recorded call must read the static batch's OWN tensors: a converted copy inside the recorded step would be swapped out
        # silently by a hand-over
        want = (frames.data_ptr(), gt2d.data_ptr() if gt2d is not None else d.head.gt2d,
                gt3d.data_ptr() if gt3d is not None else d.head.gt3d, st.data_ptr())
        if (d.mlp.x, d.head.gt2d, d.head.gt3d, d.head.skel_type) != want:
            return None
        return {'key2': key2, 'key3': key3, 'device': frames.device,
                'shapes': (tuple(frames.shape), tuple(gt2d.shape) if gt2d is not None else None,
                           tuple(gt3d.shape) if gt3d is not None else None, tuple(st.shape)),
                'static_ptrs': (d.mlp.x, d.head.gt2d, d.head.gt3d, d.head.skel_type)}

    def _hand_over(self, flow, batch) -> bool:
        """Direct replay only (the captured step is ONE recorded C-ABI call on a descriptor this trainer owns): a new batch is
        not copied into the static buffers -- the descriptor's four input addresses (frames, the two targets, the skeleton-type
        index) are pointed at the batch's own tensors and the target pairs are counted into the buffer the call reads. What the
        reference's loop does per batch -- move it to the device, run the batch-start hook (projection.py:52-71) -- is then
        one count launch; the batch object is kept alive until the next one arrives. Returns False when the batch does not
        have the static batch's exact layout on the device (the copying path then normalises it, as before)."""
        if batch is self._staged_src:
            return True
        h = self._direct.get('handover')
        if h is None:
            return False

        def refuse():                              # the copying path takes over: the call reads the static buffers again
            if self._handed_over is not None:
                d = self._direct['desc']
                d.mlp.x, d.head.gt2d, d.head.gt3d, d.head.skel_type = h['static_ptrs']
                self._handed_over = None
            return False
        try:
            frames, targets, meta = batch
            gt2d = targets[h['key2']] if h['key2'] is not None else None
            gt3d = targets[h['key3']] if h['key3'] is not None else None
            st = meta['skel_type']
        except (KeyError, TypeError, ValueError):
            return refuse()
        dev, f32 = h['device'], torch.float32
        for t, shape, dt in ((frames, h['shapes'][0], f32), (gt2d, h['shapes'][1], f32), (gt3d, h['shapes'][2], f32),
                             (st, h['shapes'][3], torch.int32)):
            if shape is None:
                continue
            if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt and tuple(t.shape) == shape
                    and t.is_contiguous() and t.data_ptr() % 16 == 0):      # (p2c_train_step_launch wants 16-byte aligned rows)
                return refuse()
        d = self._direct['desc']
        d.mlp.x, d.head.skel_type = frames.data_ptr(), st.data_ptr()
        if gt2d is not None:
            d.head.gt2d = gt2d.data_ptr()
            flow._pair_counter(gt2d)               # into flow._pair_counts_buf, the address the recorded call reads
        if gt3d is not None:
            d.head.gt3d = gt3d.data_ptr()
        self._handed_over = batch                  # keeps the tensors alive while the launches that read them run
        self._staged_src = batch
        return True

    def _capture(self, flow, batch, batch_idx):
        """Capture on the trainer's static batch (``stage_batch`` fills it; the flow's batch-start hook already ran)."""
        distributed = self.exchange is not None and self.exchange.enabled
        # the captured launches keep the ADDRESS of the per-batch skeleton-type index: it must be the static batch's own tensor
        # (stage_batch refills it in place), not a temporary the batch-start hook derived from something else
        st = batch[2].get('skel_type') if isinstance(batch[2], dict) else None
        held = getattr(getattr(flow, 'projection', None), '_skel_type', None)
        if isinstance(st, torch.Tensor) and isinstance(held, torch.Tensor) and held.data_ptr() != st.data_ptr():
            raise RuntimeError('graph capture: ProjectionModule holds a skeleton-type tensor that is not the static batch\'s '
                               f'(meta[\'skel_type\'] is {st.dtype} on {st.device}; int32 on the frames\' device is kept as is)')
        # the warm-up iterations below are real optimisation steps: snapshot parameters + optimizer state and restore
        # them IN PLACE afterwards (the graphs hold the addresses), so that replay #1 is training step #1
        snapshot = self._snapshot(flow)
        # ONE side stream for the warm-up steps and for every capture below: autograd's AccumulateGrad nodes remember the stream
        # they were created on and outlive a step whenever anything still references its graph; a node from the warm-up that
        # runs on another stream than the capture's put the gradients of the parameters that reach the flat buffer through
        # AccumulateGrad (PoseFormer's position embeddings, patch embedding, frame-mean bias) one step late in the replayed
        # graph -- found with NaN-filled torch.empty (tests/conftest.py P2C_POISON_EMPTY), visible without it as parameters that
        # drift from the eager trainer by ~lr per step
        side = self._capture_stream = torch.cuda.Stream()
        outer = torch.cuda.current_stream()
        side.wait_stream(outer)
        with torch.cuda.stream(side):                 # warm-up outside capture (allocator, lazy inits, autotuning)
            for _ in range(3):
                self._forward_backward(flow, batch, batch_idx, batch_start=False)
                if distributed:
                    # NOT on the side stream: a blocking collective runs on the stream it is issued from, and the process
                    # group's watchdog thread keeps polling its completion event for up to one more period (~100 ms) after it
                    # finished. An event last recorded on a stream that is capturing by then cannot be queried
                    # (hipErrorCapturedEvent): the watchdog throws and the process aborts. Seen once in stage A's capture below.
                    outer.wait_stream(side)
                    with torch.cuda.stream(outer):
                        self.exchange.all_reduce_gradients()
                    side.wait_stream(outer)
                self._optimizer_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        mode = os.environ.get('P2C_GRAPH_ALLREDUCE', 'auto')
        g_fb = self._new_graph(keep=distributed)
        if distributed and mode != '0':
            # the RCCL all-reduce is captured too: the whole step is ONE graph replay (one-rank rehearsal: 49 us against
            # 59 us for graph + eager collective + optimizer launch). Guarded: a failed capture / first replay on any rank,
            # or ranks whose parameters differ after that replay, send every rank to the eager-collective path below.
            if self._capture_with_allreduce(flow, batch, batch_idx, g_fb, snapshot, strict=(mode == '1')):
                return
            g_fb = self._new_graph(keep=True)
        if distributed:
            with torch.cuda.graph(g_fb, stream=side):
                self._static_loss = self._forward_backward(flow, batch, batch_idx, batch_start=False)
            if self._kept_graph:
                self._graph_nodes = self._count_nodes(g_fb)      # stage A alone: forward + backward
                g_fb.instantiate()
            if all(hasattr(o, '_descriptor') for o in self.optimizers) and self.gradient_clip_val is None:
                g_opt = 'eager'          # FlatAdamW is a single kernel: a direct launch has less latency than a 1-node graph
            else:
                g_opt = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_opt, stream=side):
                    self._optimizer_step()
        else:
            g_opt = None
            # A step that is nothing but ONE recorded C-ABI call (the two-launch train step with the optimizer inside) is
            # replayed by making that call again: a graph launch costs ~5 us of start-up per replay, two direct kernel
            # launches ~2 us of gap (B = 256: 32.6 -> see DESIGN section 5). Checked, not assumed: the call is recorded during
            # the capture and the captured graph must hold exactly its two kernel nodes. P2C_DIRECT_REPLAY=0 keeps the graph.
            from pedestrians_video_2_carla_amd import ops
            try_direct = self._opt_in_backward and os.environ.get('P2C_DIRECT_REPLAY', '1') == '1'
            rec = [] if try_direct else None
            if try_direct:
                g_fb = self._new_graph(keep=True)
                try_direct = self._kept_graph          # an older torch without keep_graph: the plain graph replays the step
                rec = rec if try_direct else None
            ops.TRAIN_STEP_RECORDER = rec
            try:
                with torch.cuda.graph(g_fb, stream=side):
                    self._static_loss = self._forward_backward(flow, batch, batch_idx, batch_start=False)
                    self._optimizer_step()
            finally:
                ops.TRAIN_STEP_RECORDER = None
            if try_direct:
                self._direct = self._direct_replay_plan(g_fb, rec)
                g_fb.instantiate()
                if self._direct is not None and os.environ.get('P2C_HAND_OVER', '1') == '1':
                    self._direct['handover'] = self._handover_info(flow, batch)
        self._graphs = (g_fb, g_opt)
        self._restore(flow, snapshot)
        if self._direct is None and not distributed and os.environ.get('P2C_VERIFY_REPLAY', '1') == '1':
            self._verify_replay(flow, snapshot)

    def _verify_replay(self, flow, snapshot):
        """(Single-GPU captures only: the distributed captures -- all-reduce in the graph, or stage A with an eager optimizer -- are
        NOT compared with an eager step here; ``ranks_agree`` only establishes that every rank holds the same bits.)
        Capture-time check: the new graph is replayed twice -- other tensors allocated, written and freed before each replay --
        and its parameter update compared with the same step issued eagerly from the same parameters and random-number state
        (a captured step draws the same philox offsets as the eager one, and the in-kernel dropout streams are put back; the build's kernels give the same bits either way:
        measured difference exactly 0 for cfg2 / cfg3 / cfg5 with dropout and stochastic depth on). A step that reads memory the
        graph does not own, or captured a stale address, shows up here; the trainer then goes back to eager steps and says so.
        NOT caught here: on this stack (PyTorch 2.10 / ROCm 7.0) a captured backward with one of the framework's multi-block
        reductions goes wrong only later, some replays and allocations into training (tools/graph_reduce_repro.py) -- the flows
        of this build keep those out of their steps, and tests/test_graph_replay_gpu.py replays with churn. P2C_VERIFY_REPLAY=0
        skips the check."""
        g_fb, g_opt = self._graphs
        state = self.flat.flat_param.data if self.flat is not None else None
        if state is None or g_opt is not None:
            return
        dev = state.device
        rng = torch.cuda.get_rng_state(dev)
        from pedestrians_video_2_carla_amd import ops
        drop = ops.dropout_states_snapshot()                 # the masks drawn inside kernels: the same stream position each time
        before = state.clone()
        # ground truth: the same step issued eagerly on the static batch, from the same parameters and random-number state (a
        # captured step draws the same philox offsets as the eager one when it starts from the same generator state)
        torch.cuda.set_rng_state(rng, dev)
        self._forward_backward(flow, self._static_batch, 0, batch_start=False)
        self._optimizer_step()
        torch.cuda.synchronize(dev)
        want = state - before
        self._restore(flow, snapshot)
        ops.dropout_states_restore(drop)
        updates = []
        for attempt in range(2):
            # what a training loop does between two steps: other tensors come and go (and leave their values behind)
            junk = [torch.empty(1 << 20, device=dev).normal_() for _ in range(32)] + [torch.empty(256, device=dev).fill_(7.0) for _ in range(256)]
            del junk
            torch.cuda.set_rng_state(rng, dev)
            g_fb.replay()
            torch.cuda.synchronize(dev)
            updates.append(state - before)
            self._restore(flow, snapshot)
            ops.dropout_states_restore(drop)
        torch.cuda.set_rng_state(rng, dev)
        scale = float(want.abs().max())
        diff = max(float((u - want).abs().max()) for u in updates)
        self._replay_check = (diff, scale)
        if not (diff <= 0.05 * scale):                       # (NaN compares false)
            print(f'[trainer] the captured step does not replay reproducibly (its update differs from the eager step\'s by {diff:.3e} '
                  f'of {scale:.3e} after other allocations): a framework reduction in its backward? Falling back to eager steps.',
                  file=sys.stderr, flush=True)
            self._graphs = None
            self._direct = None
            self.use_graph = False

    def _new_graph(self, keep: bool = False):
        """A CUDAGraph; ``keep`` asks torch to keep the captured hipGraph_t so its nodes can be counted (instantiate() is then
        ours to call). A torch without ``keep_graph`` gives the plain graph (``self._kept_graph`` False)."""
        self._kept_graph = False
        if keep:
            try:
                g = torch.cuda.CUDAGraph(keep_graph=True)
                self._kept_graph = True
                return g
            except TypeError:
                pass
        return torch.cuda.CUDAGraph()

    @staticmethod
    def _count_nodes(graph):
        import ctypes
        from pedestrians_video_2_carla_amd import _lib
        total, kernels = ctypes.c_int32(0), ctypes.c_int32(0)
        try:
            rc = _lib.lib().p2c_graph_node_counts(graph.raw_cuda_graph(), ctypes.byref(total), ctypes.byref(kernels))
        except Exception:                       # noqa: BLE001 -- no handle on this torch
            return None
        return (total.value, kernels.value) if rc == 0 else None

    @staticmethod
    def _direct_replay_plan(graph, rec):
        """The recorded call if the captured graph is exactly its launches, else None."""
        import ctypes
        from pedestrians_video_2_carla_amd import _lib
        if rec is None or len(rec) != 1:
            return None
        total, kernels = ctypes.c_int32(0), ctypes.c_int32(0)
        try:
            rc = _lib.lib().p2c_graph_node_counts(graph.raw_cuda_graph(), ctypes.byref(total), ctypes.byref(kernels))
        except Exception:                       # noqa: BLE001 -- no handle: keep the graph
            return None
        # two launches (clip kernel + weight gradient / optimizer / losses), or three at large batches (streamed weight
        # gradient + its reduction): nothing else may sit in the graph
        if rc != 0 or total.value != kernels.value or kernels.value not in (2, 3):
            return None
        plan = rec[0]
        plan['device_index'] = plan['device'].index if plan['device'].index is not None else torch.cuda.current_device()
        plan['call'] = _lib.lib().p2c_train_step
        plan['desc_ref'] = ctypes.byref(plan['desc'])
        return plan

    def _capture_with_allreduce(self, flow, batch, batch_idx, graph, snapshot, strict: bool) -> bool:
        """Capture forward + backward + all-reduce + optimizer as one graph. The ranks VOTE before anything that carries a
        collective is replayed: a rank whose capture raised never meets a healthy rank's in-graph all-reduce with its own
        eager one (collectives of different sizes pair up and the job hangs). Only when every rank captured does the
        verification replay run, followed by a second agreement on bit-identical parameters."""
        ok, err = True, None
        try:
            with torch.cuda.graph(graph, stream=self._capture_stream):
                self._static_loss = self._forward_backward(flow, batch, batch_idx, batch_start=False)
                self.exchange.all_reduce_gradients()
                self._optimizer_step()
        except Exception as e:                  # noqa: BLE001 -- any failure means "use the eager collective"
            ok, err = False, e
        torch.cuda.synchronize()                # a capture that aborted mid-way leaves nothing in flight behind it
        device = self.flat.flat_param.device if self.flat is not None else next(flow.parameters()).device
        agreed = ranks_agree(ok, device)        # eager collectives on the (non-capturing) current stream
        if agreed:
            try:
                self._graph_nodes = self._count_nodes(graph)     # (all nodes, kernel nodes) of the captured step, or None
                if self._kept_graph:
                    graph.instantiate()
                graph.replay()                  # one real step: every rank must come out with the same parameters
                torch.cuda.synchronize()
            except Exception as e:              # noqa: BLE001
                ok, err = False, e
            params = self.flat.flat_param.data if self.flat is not None else torch.cat([p.data.reshape(-1) for p in flow.parameters()])
            agreed = ranks_agree(ok, device, params.double().sum())
        self._restore(flow, snapshot)
        if agreed:
            self._graphs = (graph, None)
            return True
        if strict:
            raise RuntimeError(f'P2C_GRAPH_ALLREDUCE=1: capturing the all-reduce failed ({err!r})')
        if dist.get_rank() == 0:
            print(f'[trainer] captured all-reduce unavailable ({err!r}); using the eager collective', file=sys.stderr, flush=True)
        return False

    def _state_tensors(self, flow):
        tensors = [p.data for p in flow.parameters()] if self.flat is None else [self.flat.flat_param.data]
        tensors += [b for b in flow.buffers()]
        for o in self.optimizers:
            for st in o.state.values():
                tensors += [v for v in st.values() if isinstance(v, torch.Tensor)]
        return tensors

    def _snapshot(self, flow):
        # optimizer state is created lazily by the first step: run one throw-away step so every state tensor exists
        # and the snapshot / restore pair can work in place
        params = [t.clone() for t in self._state_tensors(flow)]
        from pedestrians_video_2_carla_amd import ops
        self._drop_pre = ops.dropout_states_snapshot()       # the streams of the in-kernel dropout masks belong to the state too
        return params

    def _restore(self, flow, snapshot):
        tensors = self._state_tensors(flow)
        with torch.no_grad():
            for t, s in zip(tensors, snapshot):          # parameters / buffers / pre-existing optimizer state
                t.copy_(s)
            for t in tensors[len(snapshot):]:            # optimizer state created during warm-up: back to step 0
                t.zero_()
            if self.flat is not None:
                self.flat.zero_grad()                    # whatever the warm-up steps left in the gradient buffer
            from pedestrians_video_2_carla_amd import ops
            ops.dropout_states_restore(getattr(self, '_drop_pre', []), rewind_new=True)   # replay #1 draws what eager step #1 would
        for m in getattr(self, '_packed', []):           # the parameters were rewritten behind the optimizer's back
            m.repack()
        torch.cuda.synchronize()

    def validate(self, flow, batches: Iterable, losses: bool = False) -> Dict[str, float]:
        """One validation epoch over ``batches`` (Lightning's hook order: ``on_validation_batch_start`` -> ``validation_step``),
        in eval mode and without gradients, issued eagerly; the flow's train / eval mode is put back afterwards. Returns the
        epoch's metrics, all-reduced over the ranks (``flow.compute_metrics(sync=True)``, which also resets them).
        ``losses=True`` returns the epoch's MONITORS instead: the batch-size-weighted mean of every ``val_loss/*`` value the
        flow logged (Lightning's ``on_epoch`` reduction, sum(v_b B_b) / sum(B_b)), accumulated on the device and read once, plus
        the metrics as ``val/<name>`` (the reference's names); the flow's per-batch state is put back as well, so a train step
        that follows -- captured or not -- is what it would have been without the validation."""
        if losses:
            return self._eval_epoch(flow, batches, 'val')
        was_training = flow.training
        flow.eval()
        try:
            with torch.no_grad():
                for i, batch in enumerate(batches):
                    flow.on_validation_batch_start(batch, i)
                    flow.validation_step(batch, i)
        finally:
            flow.train(was_training)
        return flow.compute_metrics(sync=True)

    def test(self, flow, batches: Iterable, ckpt_path: Optional[str] = None) -> Dict[str, float]:
        """The same loop with ``on_test_batch_start`` / ``test_step``: ``test_loss/*`` means and ``test/<metric>``. ``ckpt_path``:
        a checkpoint file, or ``'best'`` for the attached ``ModelCheckpoint``'s ``best_model_path``; its WEIGHTS are loaded
        (in place: legal on a live, captured trainer), nothing else of it."""
        if ckpt_path == 'best':
            ckpt_path = next((cb.best_model_path for cb in self.callbacks if getattr(cb, 'best_model_path', '')), None)
            if not ckpt_path:
                raise RuntimeError("test(ckpt_path='best') needs a ModelCheckpoint callback that has saved a checkpoint")
        if self._flow is None:                     # a trainer that was never set up: the flow still finds its data module
            flow.trainer = self
        if ckpt_path is not None:
            self.load_checkpoint(ckpt_path, weights_only=True, flow=flow)
        return self._eval_epoch(flow, batches, 'test')

    def _eval_epoch(self, flow, batches: Iterable, stage: str) -> Dict[str, float]:
        batch_start = flow.on_validation_batch_start if stage == 'val' else flow.on_test_batch_start
        step = flow.validation_step if stage == 'val' else flow.test_step
        prefix = f'{stage}_loss/'
        logged = getattr(flow, 'logged', None)
        was_training = flow.training
        projection = getattr(flow, 'projection', None)
        held = {o: {k: getattr(o, k) for k in keys if hasattr(o, k)}
                for o, keys in ((flow, ('_pair_counts',)), (projection, ('_skel_type', '_batch_size'))) if o is not None}
        sums: Dict[str, torch.Tensor] = {}
        counts: Dict[str, int] = {}
        flow.eval()
        try:
            with torch.no_grad():
                for i, batch in enumerate(batches):
                    if logged is not None:             # only what THIS batch logs is folded in
                        for k in [k for k in logged if k.startswith(prefix)]:
                            del logged[k]
                    batch_start(batch, i)
                    step(batch, i)
                    n = len(batch[0])
                    for k, v in (logged or {}).items():
                        if k.startswith(prefix) and isinstance(v, torch.Tensor) and v.ndim == 0:
                            term = v.to(torch.float64) * n            # device arithmetic in fp64: nothing is read here
                            sums[k] = term if k not in sums else sums[k] + term
                            counts[k] = counts.get(k, 0) + n
        finally:
            flow.train(was_training)
            for o, values in held.items():
                for k, v in values.items():
                    setattr(o, k, v)
        monitors: Dict[str, float] = {}
        if sums:
            names = sorted(sums)
            table = torch.stack([torch.stack([sums[k] for k in names]),
                                 torch.tensor([float(counts[k]) for k in names], dtype=torch.float64).to(sums[names[0]].device)])
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                dist.all_reduce(table, op=dist.ReduceOp.SUM)
            monitors.update(zip(names, (table[0] / table[1]).tolist()))       # the epoch's one read of the losses
        monitors.update({f'{stage}/{k}': v for k, v in flow.compute_metrics(sync=True).items()})
        self.callback_metrics = {**self.callback_metrics, **monitors}
        return monitors

    # ---- checkpoints (checkpoint.py) ----------------------------------------------------------------------------------------
    def save_checkpoint(self, path: str, flow=None) -> str:
        """Everything a resumed run needs, in one file with Lightning's top-level keys (see checkpoint.py). Rank 0 writes, all
        ranks wait. Checkpoints written by ``ModelCheckpoint`` sit on epoch boundaries; one made by hand in the middle of an
        epoch resumes at the NEXT boundary's batch order (mid-epoch data resume is out of scope)."""
        from pedestrians_video_2_carla_amd import checkpoint
        return checkpoint.save(self, flow if flow is not None else self._flow, path)

    def load_checkpoint(self, path: str, weights_only: bool = False, flow=None) -> dict:
        """Full load (weights, optimizer, schedulers, callbacks, counters, dropout streams, generators): only on a trainer that
        was set up and has not stepped -- anything else raises, nothing is half-restored. ``weights_only=True``: parameters and
        buffers in place plus re-packed weight images, legal at any time."""
        from pedestrians_video_2_carla_amd import checkpoint
        flow = flow if flow is not None else self._flow
        if flow is None:
            raise RuntimeError('load_checkpoint needs the flow: call setup() first or pass flow=')
        ckpt = checkpoint.load(self, flow, path, weights_only=weights_only)
        if not weights_only:
            self._loaded_p2c = ckpt.get(checkpoint.P2C_KEY) or {}
        return ckpt

    def predict(self, flow, batches: Iterable) -> List:
        """Lightning's predict loop over ``batches``: ``flow.predict_step(batch, i)`` (which runs the batch-start hook itself) in
        eval mode and without gradients, issued eagerly; the flow's train / eval mode is put back afterwards. Returns the list
        of ``(sliced, meta)`` -- what ``BaseDataModule.save_predictions`` and ``save_carla_animation`` take."""
        was_training = flow.training
        flow.eval()
        try:
            with torch.no_grad():
                return [flow.predict_step(batch, i) for i, batch in enumerate(batches)]
        finally:
            flow.train(was_training)

    def predict_carla(self, flow, batches: Iterable, ik: bool = False, src_fps=None, out_fps=None, smooth=None,
                      root_motion=None, loop=None) -> List:
        """The predict loop for a CARLA player: per batch ``(bones (B,T,26,6), root (B,T,6), meta)``, the rows
        ``export_clips(flow.predict_step(batch))`` would give, left on the batch's device. A LinearAE flow takes one launch per
        batch (K32, ``walker_control.carla_lifter.CarlaLifter``); other movements models the composed path. A movements model
        that outputs absolute locations has no bone rotations to export and raises ``KeyError``; with ``ik=True`` such a flow
        goes through ``walker_control.location_retargeter.LocationRetargeter`` instead: model -> pose head -> the rotations
        fitted to the predicted locations (K36, one launch per batch). ``src_fps`` and ``out_fps``, given together: every
        clip's rows are resampled from the one rate to the other where they are (``CarlaResampler.resample``, K37: one more
        launch per batch), so T becomes the clip's output count. ``smooth``: a ``CarlaSmoother`` or a dict of its arguments; every
        clip's rows are smoothed along time as a video of its own (``CarlaSmoother.smooth``, K39: one more launch per batch)
        before any resampling (a dict for ``one_euro`` without ``fps`` takes ``src_fps``). ``root_motion``: True, a
        ``CarlaRootMotion`` or a dict of its arguments; every clip, a video of its own, gets root rows that keep its supporting
        foot planted (``CarlaRootMotion.apply``, K40: one more launch per batch), after the smoothing and before any resampling.
        ``loop``: a ``CarlaLooper`` that knows its ``frames`` or a dict of its arguments with ``frames``; every clip, a video of its
        own, becomes that many frames of the cycle that closes best (``CarlaLooper.loop``, K41), after the root motion and before
        any resampling, so T becomes ``frames``.
        Eval mode, no gradients, the flow's train / eval mode is put back afterwards."""
        from pedestrians_video_2_carla_amd.walker_control.carla_lifter import CarlaLifter
        if (src_fps is None) != (out_fps is None):
            raise ValueError('predict_carla: src_fps and out_fps come together or not at all')
        if out_fps is None:
            rate = lambda bones, root: (bones, root)                               # noqa: E731
        else:
            from pedestrians_video_2_carla_amd.walker_control.resample import CarlaResampler
            rate = CarlaResampler(src_fps, out_fps).resample
        if loop is not None:
            from pedestrians_video_2_carla_amd.walker_control.loop import as_looper
            looper, then = as_looper(loop), rate
            rate = lambda bones, root: then(*looper.loop(bones, root))                 # noqa: E731
        if root_motion is not None:
            from pedestrians_video_2_carla_amd.walker_control.root_motion import as_root_motion
            mover, after = as_root_motion(root_motion), rate
            if mover is not None:
                rate = lambda bones, root: after(*mover.apply(bones, root))            # noqa: E731
        if smooth is not None:
            from pedestrians_video_2_carla_amd.walker_control.smooth import as_smoother
            smoother, resample = as_smoother(smooth, src_fps), rate
            rate = lambda bones, root: resample(*smoother.smooth(bones, root))     # noqa: E731
        lifter = CarlaLifter(flow)
        was_training = flow.training
        flow.eval()
        try:
            with torch.no_grad():
                if ik and lifter.kind is None:
                    from pedestrians_video_2_carla_amd.walker_control.location_retargeter import LocationRetargeter
                    fit = LocationRetargeter()
                    fit.check_flow(flow)
                    return [(*rate(*fit.lift(flow, batch)), batch[2]) for batch in batches]
                return [(*rate(*lifter.lift(batch[0], batch[2])), batch[2]) for batch in batches]
        finally:
            flow.train(was_training)
            lifter.close()

    def _video_writers(self) -> List:
        """The writers of the attached ``PedestrianLogger``s that write at all (none attached: the loggers module is not imported)."""
        if not self.loggers:
            return []
        from pedestrians_video_2_carla_amd.loggers.pedestrian import PedestrianLogger
        return [lg.experiment for lg in self.loggers if isinstance(lg, PedestrianLogger) and not lg.disabled]

    def _log_train_videos(self, flow, batch, step: int, writers: List) -> None:
        """Training clips. The reference logs the train-mode outputs of the step itself; here the lean train step returns no
        projection and a replayed graph runs no Python, so after a step whose index passes a writer's gate the batch goes through
        ONE extra forward (``flow.predict_step``: eval mode, no gradients -- no dropout stream and no BatchNorm statistic moves),
        logged as stage ``train``. The flow's mode and per-batch state are put back: the training steps are what they are without a
        logger."""
        writers = [w for w in writers if w.wants(step)]
        if not writers:
            return
        was_training = flow.training
        projection = getattr(flow, 'projection', None)
        held = {o: {k: getattr(o, k) for k in keys if hasattr(o, k)}
                for o, keys in ((flow, ('_pair_counts',)), (projection, ('_skel_type', '_batch_size'))) if o is not None}
        flow.eval()
        try:
            with torch.no_grad():
                sliced, meta = flow.predict_step(batch, step)
                for w in writers:
                    w.log_videos(meta=meta, step=step, batch_idx=step, stage='train', inputs=sliced.get('inputs'),
                                 targets=sliced.get('targets'), projection_2d=sliced.get('projection_2d'),
                                 projection_2d_transformed=sliced.get('projection_2d_transformed'))
        finally:
            flow.train(was_training)
            for o, values in held.items():
                for k, v in values.items():
                    setattr(o, k, v)

    def fit(self, flow, datamodule, batches: Optional[Iterable] = None, val_batches=None, ckpt_path: Optional[str] = None):
        """``max_steps`` steps over ``batches`` (or the data module's), as before -- or, with any of ``max_epochs``,
        ``val_batches``, ``callbacks``, ``ckpt_path`` given (or ``steps_per_epoch`` and a data module with ``val_batches``), the
        epoch loop (``_fit_epochs``). Returns the per-step losses (device tensors) of this call."""
        self.setup(flow, datamodule)
        device = self.device or flow.device
        if val_batches is None and hasattr(datamodule, 'val_batches') and (self.steps_per_epoch or self.max_epochs is not None):
            val_batches = datamodule.val_batches(device)
        if self.max_epochs is not None or val_batches is not None or self.callbacks or ckpt_path is not None:
            return self._fit_epochs(flow, datamodule, batches, val_batches, ckpt_path)
        if batches is None:
            rank = dist.get_rank() if dist.is_initialized() else 0
            batches = datamodule.train_batches(device, self.max_steps, rank=rank)
        losses = []
        writers = self._video_writers()
        for i, batch in enumerate(batches):
            if i >= self.max_steps:
                break
            losses.append(self.train_step(flow, batch, i))
            if writers:
                self._log_train_videos(flow, batch, i, writers)
            if self.log_every_n_steps and (i + 1) % self.log_every_n_steps == 0:
                flow.check_finite('train')
            if self.steps_per_epoch and (i + 1) % self.steps_per_epoch == 0:
                self.current_epoch += 1
                self.step_lr_schedulers('epoch', {k: float(v) for k, v in getattr(flow, 'logged', {}).items()
                                                  if isinstance(v, (float, int)) or (isinstance(v, torch.Tensor) and v.ndim == 0)})
        return losses

    # ---- the epoch loop ------------------------------------------------------------------------------------------------------
    def _fit_epochs(self, flow, datamodule, batches, val_batches, ckpt_path) -> List[torch.Tensor]:
        """Epochs of ``steps_per_epoch`` steps of ``batches`` -- or one pass over a sized re-iterable (a ``DeviceLoader``, a list)
        per epoch. End of an epoch, in this order: (1) validation, every ``check_val_every_n_epoch`` epochs; (2) the
        epoch-interval LR schedulers, with this epoch's monitors; (3) the callbacks' ``on_validation_end``. A checkpoint written
        in (3) therefore holds the scheduler state the next epoch starts from, which is what makes resuming exact.
        ``ckpt_path``: full load right after ``setup`` (the trainer has not stepped), then training goes on from the stored
        epoch and step."""
        device = self.device or flow.device
        sized = batches is not None and hasattr(batches, '__len__') and not hasattr(batches, '__next__')
        self._train_batches = batches if sized else None
        if ckpt_path is not None:
            self.load_checkpoint(ckpt_path, flow=flow)
            epoch = getattr(self, '_loaded_p2c', {}).get('loader_epoch')
            if sized and epoch is not None and hasattr(batches, 'epoch'):
                batches.epoch = epoch              # the loader's shuffle order is a function of it
        if not sized and not self.steps_per_epoch:
            raise ValueError('the epoch loop needs steps_per_epoch, or batches with a length that can be iterated once per epoch')
        per_epoch = min(len(batches), self.steps_per_epoch or len(batches)) if sized else self.steps_per_epoch
        limits = [n for n in (self.max_steps, self.max_epochs * per_epoch if self.max_epochs is not None else None)
                  if n is not None and n >= 0]
        if not limits:
            raise ValueError('the epoch loop needs max_epochs or max_steps')
        total = min(limits)
        stream = None
        if not sized:
            if batches is None:
                rank = dist.get_rank() if dist.is_initialized() else 0
                batches = datamodule.train_batches(device, max(total - self.global_step, 0), rank=rank, first_step=self.global_step)
            stream = iter(batches)
        losses: List[torch.Tensor] = []
        writers = self._video_writers()
        # a checkpoint made by hand inside an epoch: the rest of that epoch first, so the next boundary is where it would have been
        carry = min(max(self.global_step - self.current_epoch * per_epoch, 0), per_epoch - 1)
        while self.global_step < total:
            source = iter(batches) if sized else stream
            done, carry = carry, 0
            for batch in source:
                i = self.global_step
                losses.append(self.train_step(flow, batch, i))
                if writers:
                    self._log_train_videos(flow, batch, i, writers)
                if self.log_every_n_steps and (i + 1) % self.log_every_n_steps == 0:
                    flow.check_finite('train')
                done += 1
                if done >= per_epoch or self.global_step >= total:
                    break
            if done < per_epoch:
                if done == 0 or self.global_step >= total or not sized:
                    break                          # out of batches, or max_steps ended the run inside an epoch: no epoch end
            self._end_epoch(flow, val_batches, device)
        for cb in self.callbacks:
            if hasattr(cb, 'on_fit_end'):
                cb.on_fit_end(self, flow)
        return losses

    def _end_epoch(self, flow, val_batches, device) -> None:
        self.current_epoch += 1
        validated = val_batches is not None and self.current_epoch % self.check_val_every_n_epoch == 0
        if validated:
            source = val_batches(device) if callable(val_batches) else val_batches
            self._eval_epoch(flow, source, 'val')
        # Lightning hands a plateau scheduler the last value logged under its key: this epoch's validation mean, the last one
        # in an epoch without validation, or a training value the flow logged (read only when a scheduler asks for it)
        monitors = dict(self.callback_metrics)
        for sched in self.lr_schedulers:
            key = sched.get('monitor')
            value = getattr(flow, 'logged', {}).get(key) if key is not None and key not in monitors else None
            if isinstance(value, (float, int)) or (isinstance(value, torch.Tensor) and value.ndim == 0):
                monitors[key] = float(value)
        self.step_lr_schedulers('epoch', monitors)
        if validated:
            for cb in self.callbacks:
                if hasattr(cb, 'on_validation_end'):
                    cb.on_validation_end(self, flow, dict(self.callback_metrics))
