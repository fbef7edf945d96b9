"""``FlatAdamW``: torch.optim.AdamW / Adam semantics, one HIP launch over the flat parameter buffer.

The reference configures ``torch.optim.AdamW(self.parameters(), lr, weight_decay)`` (modules/flow/base_model.py:156-158).
With every parameter a view of one flat buffer (parallel/flat.py) the step is a single element-wise pass
(``p2c_adamw_step``, csrc/p2c_optim.hip). Differences from handing the flat tensor to torch's fused AdamW:
  * step counter and hyper-parameters live in device memory -> the launch can be captured in a HIP graph and still follow
    an LR scheduler (``param_groups[0]['lr']`` is re-uploaded when it changes);
  * the 1/world_size gradient averaging of data-parallel training (``grad_scale``) and next step's ``zero_grad`` are
    folded into the same pass;
  * ``set_clip`` folds torch.nn.utils.clip_grad_norm_ / clip_grad_value_ into it as well (K29, csrc/p2c_grad_clip.hip): the
    norm is reduced on the device, never read on the host, and the launches stay capturable.
``state_dict()`` has torch's layout (``step``, ``exp_avg``, ``exp_avg_sq``) for ONE flat parameter: it is interchangeable with a
torch.optim.AdamW built over the same flat tensor, NOT with the reference's per-parameter optimizer state (there the moments
are one pair per module parameter; slicing the flat moments by ``FlatParameters.params`` offsets converts between the two).
"""
import ctypes

import torch

from pedestrians_video_2_carla_amd import _lib


class FlatAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True,
                 zero_grad_in_step=True):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        ps = [p for g in self.param_groups for p in g['params']]
        if len(self.param_groups) != 1 or len(ps) != 1:
            raise ValueError('FlatAdamW optimises exactly one flat parameter tensor')
        (p,) = ps
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise _lib.P2CError('FlatAdamW needs a contiguous fp32 parameter on the GPU (there is no CPU fallback)')
        self.decoupled = bool(decoupled)
        self.zero_grad_in_step = bool(zero_grad_in_step)
        self.grad_scale = 1.0
        self.fused_steps_applied = 0              # bumped by every backward that applied this optimizer's step itself
        self._uploaded = None
        self._scatter = None                      # (int32 index per parameter, destination buffer) or None
        self._clip = None                         # (mode, bound) or None
        self._clip_partials = None                # norm mode: one double per workgroup of the squared-norm launch
        self.last_grad_norm = None                # norm mode: device scalar, the last step's total norm (never synced)
        self._hyper = torch.zeros(6, dtype=torch.float32, device=p.device)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=p.device)
        self.state[p] = {'step': torch.zeros((), dtype=torch.float32, device=p.device),
                         'exp_avg': torch.zeros_like(p, memory_format=torch.preserve_format),
                         'exp_avg_sq': torch.zeros_like(p, memory_format=torch.preserve_format)}

    def load_state_dict(self, state_dict):
        """torch leaves ``state['step']`` where the loaded dict had it (a host tensor for a checkpoint read with
        ``map_location='cpu'`` or for the state of a plain torch.optim.AdamW): the kernels read the counter through a device
        pointer, so all three state tensors are brought to the parameter's device here, the counter as a 0-dim fp32 tensor."""
        super().load_state_dict(state_dict)
        (p,) = self.param_groups[0]['params']
        st = self.state[p]
        step = st.get('step', 0.0)
        if isinstance(step, torch.Tensor):
            step = step.detach().to(device=p.device, dtype=torch.float32).reshape(()).clone()
        else:
            step = torch.tensor(float(step), dtype=torch.float32, device=p.device)
        st['step'] = step
        for k in ('exp_avg', 'exp_avg_sq'):
            t = st.get(k)
            if not isinstance(t, torch.Tensor) or t.shape != p.shape:
                if t is not None:
                    raise ValueError(f'FlatAdamW.load_state_dict: {k} does not have the flat parameter\'s shape')
                t = torch.zeros_like(p, memory_format=torch.preserve_format)
            st[k] = t.detach().to(device=p.device, dtype=torch.float32).contiguous()
        self._uploaded = None                     # the loaded param_groups are uploaded by the next sync_hyper()

    def set_scatter(self, index: torch.Tensor, dst: torch.Tensor):
        """After every step, parameter i is also written to ``dst[index[i]]`` (index < 0: not copied)."""
        (p,) = self.param_groups[0]['params']
        if index.numel() != p.numel() or index.dtype != torch.int32 or not index.is_cuda or not dst.is_cuda:
            raise ValueError('scatter index: one int32 per parameter, on the device')
        self._scatter = (index.contiguous(), dst)

    def set_clip(self, value, algorithm: str = 'norm'):
        """Clip the gradient inside the optimizer launch: ``'norm'`` = clip_grad_norm_(max_norm=value) (2-norm of the whole
        flat gradient, after the ``grad_scale`` averaging), ``'value'`` = clip_grad_value_(clip_value=value). ``None`` / ``0``
        turn it off. The bound is a host value: a graph captured with it keeps it."""
        if algorithm not in ('norm', 'value'):
            raise ValueError(f"gradient clip algorithm must be 'norm' or 'value', not {algorithm!r}")
        if value is None or float(value) == 0.0:
            self._clip, self.last_grad_norm = None, None
            return
        value = float(value)
        if not (value > 0.0 and value != float('inf')):
            raise ValueError(f'gradient clip value must be finite and positive, not {value!r}')
        (p,) = self.param_groups[0]['params']
        if algorithm == 'norm':
            n_partials = int(_lib.lib().p2c_grad_clip_partials(p.numel()))
            if self._clip_partials is None or self._clip_partials.numel() < n_partials:
                self._clip_partials = torch.empty(max(n_partials, 1), dtype=torch.float64, device=p.device)
            if self.last_grad_norm is None:
                self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=p.device)
            self._clip = (_lib.P2C_CLIP_NORM, value)
        else:
            self._clip, self.last_grad_norm = (_lib.P2C_CLIP_VALUE, value), None

    def _clip_descriptor(self):
        key = (self._clip, None if self._clip_partials is None else self._clip_partials.data_ptr(),
               None if self.last_grad_norm is None else self.last_grad_norm.data_ptr())
        if getattr(self, '_clip_desc_key', None) != key:
            c = _lib.ClipDesc()
            c.mode, c.bound = self._clip
            if c.mode == _lib.P2C_CLIP_NORM:
                c.partials, c.total_norm = self._clip_partials.data_ptr(), self.last_grad_norm.data_ptr()
            self._clip_desc, self._clip_desc_key = c, key
        return self._clip_desc

    def _descriptor(self, p):
        """The launch descriptor only holds addresses of long-lived buffers: built once, rebuilt if one of them moves."""
        st = self.state[p]
        key = (p.data_ptr(), p.grad.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), st['step'].data_ptr(),
               None if self._scatter is None else (self._scatter[0].data_ptr(), self._scatter[1].data_ptr()),
               self.decoupled, self.zero_grad_in_step)
        if getattr(self, '_desc_key', None) != key:
            d = _lib.AdamWDesc()
            d.n = p.numel()
            d.param, d.grad = p.data_ptr(), p.grad.data_ptr()
            d.exp_avg, d.exp_avg_sq, d.step = st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), st['step'].data_ptr()
            d.ticket, d.hyper = self._ticket.data_ptr(), self._hyper.data_ptr()
            d.adamw, d.zero_grad = int(self.decoupled), int(self.zero_grad_in_step)
            if self._scatter is not None:
                d.scatter_idx, d.scatter_dst = self._scatter[0].data_ptr(), self._scatter[1].data_ptr()
            self._desc, self._desc_key = d, key
        return self._desc

    def descriptor_for_fusion(self):
        """Launch descriptor for a kernel that applies this optimizer's step itself (p2c_mlp_desc.fused_adamw)."""
        (p,) = self.param_groups[0]['params']
        if self._clip is not None:
            raise RuntimeError('FlatAdamW: a gradient clip is set; a fused update cannot honour it (the norm has to be known '
                               'before the first parameter is touched)')
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        elif self._uploaded is None:
            raise RuntimeError('FlatAdamW: call sync_hyper() (or one eager step) before capturing a graph')
        return self._descriptor(p)

    def sync_hyper(self):
        """Upload lr / betas / eps / weight_decay / grad_scale if they changed on the host (call outside graph replay)."""
        g = self.param_groups[0]
        values = (float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']),
                  float(self.grad_scale))
        if values != self._uploaded:
            self._hyper.copy_(torch.tensor(values, dtype=torch.float32))
            self._uploaded = values

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        (p,) = self.param_groups[0]['params']
        if p.grad is None:
            return loss
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        elif self._uploaded is None:
            raise RuntimeError('FlatAdamW: call sync_hyper() (or one eager step) before capturing a graph')
        d = self._descriptor(p)
        with torch.cuda.device(p.device):
            stream = torch.cuda.current_stream(p.device).cuda_stream
            if self._clip is not None:
                _lib.check(_lib.lib().p2c_adamw_step_clipped(ctypes.byref(d), ctypes.byref(self._clip_descriptor()), stream),
                           'p2c_adamw_step_clipped')
            else:
                _lib.check(_lib.lib().p2c_adamw_step(ctypes.byref(d), stream), 'p2c_adamw_step')
        return loss
