"""Checkpoints: one ``torch.save`` file with Lightning's top-level keys, plus what no ``state_dict`` carries.

The reference resumes through Lightning (modeling.py:240-299: ``ModelCheckpoint`` writes, ``--ckpt_path`` reads). The file here has
the same top-level layout -- ``epoch``, ``global_step``, ``state_dict`` (the flow's, host tensors, the reference's key names),
``optimizer_states``, ``lr_schedulers``, ``hyper_parameters``, ``callbacks`` -- so either side can read the other's weights and
optimizer state, and ONE extra key, ``p2c``, with the state that makes a step of this build reproducible:

  * ``dropout``: the four words of every in-kernel dropout stream (``ops.dropout_state``), keyed by the owning module's dotted name;
  * ``rng_cpu`` / ``rng_cuda``: the framework generators (some dropout sites draw from philox; every new dropout stream takes one
    CPU draw for its seed);
  * ``fused_steps_applied``: FlatAdamW's count of steps applied inside a backward (the trainer compares against it);
  * ``clip``: the trainer's gradient-clip settings, checked on load;
  * ``loader_epoch``: the ``epoch`` of a ``DeviceLoader`` (its shuffle order is a function of it).

``optimizer_states`` is written in the reference's PER-PARAMETER layout: torch AdamW state indexed by the position of the
parameter in the optimizer the plugin configured, ``step`` repeated, the moments sliced out of the flat buffers at
``FlatParameters``' offsets. Loading takes that layout or the flat one-parameter layout of ``FlatAdamW.state_dict()``.

A FULL load is for a trainer that has not stepped (``Trainer.fit(ckpt_path=...)`` right after ``setup``): after a capture the
moment tensors' addresses are part of the recorded step and ``load_state_dict`` replaces them. ``weights_only=True`` copies
parameters and buffers IN PLACE and re-packs weight images; it is legal on a live, captured trainer.
"""
import enum
import os
from typing import Any, Dict, List

import torch
import torch.distributed as dist

P2C_KEY = 'p2c'


# ---- optimizer state: flat <-> per parameter ------------------------------------------------------------------------------
def _flat_offsets(flat) -> Dict[int, tuple]:
    """id(parameter) -> (offset, numel) in the flat buffers."""
    out, off = {}, 0
    for p in flat.params:
        out[id(p)] = (off, p.numel())
        off += p.numel()
    return out


def _reference_group_template(decoupled: bool) -> Dict[str, Any]:
    """The ``param_groups[0]`` keys (and defaults) of the optimizer the reference configures, from torch itself."""
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    g = dict(cls([torch.zeros(1, requires_grad=True)]).param_groups[0])
    g.pop('params')
    return g


def optimizer_state_per_parameter(flat, optimizer, ref_params: List[torch.nn.Parameter]) -> Dict[str, Any]:
    """``optimizer`` (FlatAdamW, or a torch optimizer over ``flat.flat_param``) -> the ``state_dict()`` of the same optimizer
    class built over ``ref_params`` (the parameters in the order the plugin handed them to its own optimizer). A parameter that
    is not in the flat buffer (``p2c_unused``: its gradient is always None) has no state, as in torch."""
    sd = optimizer.state_dict()
    (group,) = sd['param_groups']
    flat_state = sd['state'].get(group['params'][0], {})
    template = _reference_group_template(getattr(optimizer, 'decoupled', isinstance(optimizer, torch.optim.AdamW)))
    new_group = {**template, **{k: v for k, v in group.items() if k != 'params'}}
    new_group['params'] = list(range(len(ref_params)))
    offsets = _flat_offsets(flat)
    state = {}
    stepped = 'step' in flat_state and float(flat_state['step']) > 0
    if stepped:
        step = flat_state['step']
        step = step.detach().to('cpu', torch.float32).reshape(()) if isinstance(step, torch.Tensor) \
            else torch.tensor(float(step), dtype=torch.float32)
        for i, p in enumerate(ref_params):
            if id(p) not in offsets:
                continue
            off, n = offsets[id(p)]
            entry = {'step': step.clone()}
            for k, v in flat_state.items():
                if isinstance(v, torch.Tensor) and v.numel() == flat.numel and k != 'step':
                    entry[k] = v.detach().reshape(-1)[off:off + n].to('cpu').reshape(p.shape).clone()
            state[i] = entry
    return {'state': state, 'param_groups': [new_group]}


def optimizer_state_flat(state_dict: Dict[str, Any], flat, optimizer, ref_params: List[torch.nn.Parameter]) -> Dict[str, Any]:
    """The inverse: a per-parameter ``state_dict`` (or one that is flat already) -> what ``optimizer.load_state_dict`` takes."""
    (group,) = state_dict['param_groups']
    state = state_dict['state']
    own = optimizer.state_dict()['param_groups'][0]
    new_group = {k: group.get(k, v) for k, v in own.items() if k != 'params'}
    if 'initial_lr' in group:
        new_group['initial_lr'] = group['initial_lr']
    new_group['params'] = [0]
    if len(group['params']) == 1:
        only = state.get(group['params'][0], {})
        moment = next((v for k, v in only.items() if k != 'step' and isinstance(v, torch.Tensor)), None)
        if moment is None or moment.numel() == flat.numel:         # the flat layout of FlatAdamW.state_dict() itself
            flat_entry = {k: (v.detach().clone().reshape(-1) if isinstance(v, torch.Tensor) and k != 'step' else v)
                          for k, v in only.items()}
            return {'state': {0: flat_entry} if flat_entry else {}, 'param_groups': [new_group]}
    if len(group['params']) != len(ref_params):
        raise ValueError(f'optimizer state for {len(group["params"])} parameters, the model has {len(ref_params)}')
    offsets = _flat_offsets(flat)
    entry: Dict[str, Any] = {}
    steps = set()
    for pos, key in enumerate(group['params']):
        st, p = state.get(key), ref_params[pos]
        if not st:
            continue
        if id(p) not in offsets:
            raise ValueError(f'optimizer state for parameter {pos}, which is not optimised here')
        off, n = offsets[id(p)]
        steps.add(float(st['step']))
        for k, v in st.items():
            if k == 'step' or not isinstance(v, torch.Tensor):
                continue
            if v.numel() != n:
                raise ValueError(f'optimizer state {k!r} of parameter {pos} has {v.numel()} elements, the parameter {n}')
            buf = entry.setdefault(k, torch.zeros(flat.numel, dtype=torch.float32))
            buf[off:off + n] = v.detach().reshape(-1).to('cpu', torch.float32)
    if len(steps) > 1:
        raise ValueError(f'the parameters\' step counters differ ({sorted(steps)}): one flat optimizer cannot resume from that')
    if steps:
        entry['step'] = torch.tensor(steps.pop(), dtype=torch.float32)
    return {'state': {0: entry} if entry else {}, 'param_groups': [new_group]}


# ---- in-kernel dropout streams -------------------------------------------------------------------------------------------
def dropout_words(flow) -> Dict[str, torch.Tensor]:
    return {name: m._drop_state.detach().to('cpu').clone() for name, m in flow.named_modules()
            if isinstance(getattr(m, '_drop_state', None), torch.Tensor)}


def restore_dropout_words(flow, words: Dict[str, torch.Tensor], device) -> None:
    """A module without a stream yet gets one through its own lazy getter (one CPU draw: restore the generators AFTER this)."""
    modules = dict(flow.named_modules())
    for name, saved in words.items():
        m = modules.get(name)
        if m is None or not hasattr(m, '_kernel_drop_state'):
            raise KeyError(f'checkpoint holds a dropout stream for {name!r}, which this flow does not have')
        st = m._kernel_drop_state(torch.device(device))
        if st is not None:                    # (None: the framework's dropout was asked for, P2C_TORCH_DROPOUT=1)
            st.copy_(saved.to(st.device))


# ---- the file ------------------------------------------------------------------------------------------------------------
def _plain(value):
    """hyper-parameters as plain data: enums by name, classes by name."""
    if isinstance(value, enum.Enum):
        return value.name
    if isinstance(value, type):
        return value.__name__
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if isinstance(value, torch.Tensor):
        return value.detach().cpu()
    return value


def _loader_of(trainer):
    loader = getattr(trainer, '_train_batches', None)
    return loader if isinstance(getattr(loader, 'epoch', None), int) else None


def build_checkpoint(trainer, flow) -> Dict[str, Any]:
    if not trainer.optimizers:
        raise RuntimeError('save_checkpoint needs a trainer that was set up (Trainer.setup / fit)')
    device = trainer.device or flow.device
    optimizer_states = []
    for opt in trainer.optimizers:
        if trainer.flat is not None:
            optimizer_states.append(optimizer_state_per_parameter(trainer.flat, opt, trainer._ref_params))
        else:
            optimizer_states.append(opt.state_dict())
    datamodule = trainer.datamodule
    hyper_parameters = _plain(dict(flow.hparams))
    # the flow merges its plugins' hparams and a later plugin's unset ``input_nodes`` hides the movements model's (the
    # reference's merge does the same): written out, so that the models can be rebuilt from the file alone
    nodes = getattr(getattr(flow, 'movements_model', None), 'input_nodes', None)
    if hyper_parameters.get('input_nodes') is None and nodes is not None:
        hyper_parameters['input_nodes'] = _plain(flow.movements_model.hparams.get('input_nodes'))
    p2c = {
        'dropout': dropout_words(flow),
        'rng_cpu': torch.get_rng_state(),
        'rng_cuda': torch.cuda.get_rng_state(device) if torch.device(device).type == 'cuda' else None,
        'fused_steps_applied': getattr(trainer.optimizers[0], 'fused_steps_applied', 0),
        'clip': (trainer.gradient_clip_val, trainer.gradient_clip_algorithm),
        'loader_epoch': getattr(_loader_of(trainer), 'epoch', None),
        'steps_per_epoch': trainer.steps_per_epoch,
    }
    return {
        'epoch': trainer.current_epoch,
        'global_step': trainer.global_step,
        'pytorch-lightning_version': None,
        'state_dict': {k: v.detach().to('cpu').clone() for k, v in flow.state_dict().items()},
        'optimizer_states': optimizer_states,
        'lr_schedulers': [s['scheduler'].state_dict() for s in trainer.lr_schedulers],
        'hyper_parameters': hyper_parameters,
        'datamodule_hyper_parameters': _plain(dict(getattr(datamodule, 'hparams', None) or {})),
        'callbacks': {type(cb).__name__: cb.state_dict() for cb in trainer.callbacks if hasattr(cb, 'state_dict')},
        P2C_KEY: p2c,
    }


def _rank() -> int:
    return dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0


def save(trainer, flow, path: str) -> str:
    """Rank 0 writes (to a temporary name first: a reader never sees half a file), then a barrier."""
    if _rank() == 0:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = f'{path}.tmp'
        torch.save(build_checkpoint(trainer, flow), tmp)
        os.replace(tmp, path)
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    return path


def read(path: str) -> Dict[str, Any]:
    return torch.load(path, map_location='cpu', weights_only=False)


def load_weights(trainer, flow, checkpoint: Dict[str, Any]) -> None:
    """Parameters and buffers IN PLACE (``load_state_dict`` copies into the tensors that are there: views of the flat buffer stay
    views, a captured step keeps reading the same addresses), then every packed weight image is rebuilt."""
    with torch.no_grad():
        flow.load_state_dict(checkpoint['state_dict'], strict=True)
    for m in flow.modules():
        if m in getattr(trainer, '_packed', []) or (getattr(m, '_image_managed', False) and hasattr(m, 'repack')):
            m.repack()


def load(trainer, flow, path: str, weights_only: bool = False) -> Dict[str, Any]:
    checkpoint = read(path)
    if weights_only:
        load_weights(trainer, flow, checkpoint)
        return checkpoint
    if trainer.global_step != 0 or trainer._graphs is not None:
        raise RuntimeError('a full checkpoint load needs a trainer that has not taken a train step (fit(ckpt_path=...) loads right '
                           'after setup): the step that was captured holds the addresses of the optimizer state this would '
                           'replace. Use load_checkpoint(path, weights_only=True) on a live trainer.')
    if not trainer.optimizers:
        raise RuntimeError('load_checkpoint needs a trainer that was set up (Trainer.setup / fit)')
    extra = checkpoint.get(P2C_KEY) or {}
    clip = extra.get('clip')
    if clip is not None and tuple(clip) != (trainer.gradient_clip_val, trainer.gradient_clip_algorithm) \
            and (clip[0] is not None or trainer.gradient_clip_val is not None):
        raise RuntimeError(f'the checkpoint was trained with gradient clip {tuple(clip)}, this trainer has '
                           f'{(trainer.gradient_clip_val, trainer.gradient_clip_algorithm)}')
    load_weights(trainer, flow, checkpoint)
    for opt, state in zip(trainer.optimizers, checkpoint.get('optimizer_states', [])):
        if trainer.flat is not None:
            state = optimizer_state_flat(state, trainer.flat, opt, trainer._ref_params)
        opt.load_state_dict(state)
        if hasattr(opt, 'fused_steps_applied'):
            opt.fused_steps_applied = int(extra.get('fused_steps_applied', opt.fused_steps_applied))
            trainer._fused_seen = opt.fused_steps_applied
    for sched, state in zip(trainer.lr_schedulers, checkpoint.get('lr_schedulers', [])):
        sched['scheduler'].load_state_dict(state)
    for cb in trainer.callbacks:
        state = (checkpoint.get('callbacks') or {}).get(type(cb).__name__)
        if state is not None and hasattr(cb, 'load_state_dict'):
            cb.load_state_dict(state)
    trainer.current_epoch = int(checkpoint.get('epoch', 0))
    trainer.global_step = int(checkpoint.get('global_step', 0))
    flow.global_step = trainer.global_step
    device = trainer.device or flow.device
    restore_dropout_words(flow, extra.get('dropout') or {}, device)
    # the generators LAST: creating a dropout stream above took a CPU draw
    if extra.get('rng_cpu') is not None:
        torch.set_rng_state(extra['rng_cpu'])
    if extra.get('rng_cuda') is not None and torch.device(device).type == 'cuda':
        torch.cuda.set_rng_state(extra['rng_cuda'], device)
    # a captured trainer runs warm-up steps before its first replay; they draw from the generators again
    trainer._rng_after_capture = (extra.get('rng_cpu'), extra.get('rng_cuda'))
    return checkpoint


def load_from_checkpoint(flow_cls, checkpoint_path: str, map_location=None, **overrides):
    """``LitBaseFlow.load_from_checkpoint``: the flow is built from the file's ``hyper_parameters`` -- explicit keyword arguments
    win, as in the reference, where the command line is passed on top (modeling.py:256-260) -- and takes ``state_dict``. A model
    not given (``movements_model=...``) is built from ``{type}_model_name`` through ``flow_cls.get_available_models()``."""
    checkpoint = read(checkpoint_path)
    hparams = dict(checkpoint.get('hyper_parameters') or {})
    dm_hparams = checkpoint.get('datamodule_hyper_parameters') or {}
    if 'transform' in dm_hparams:
        hparams.setdefault('transform', dm_hparams['transform'])
    kwargs = {**hparams, **overrides}
    for model_type, choices in flow_cls.get_available_models().items():
        if kwargs.get(f'{model_type}_model') is None:
            name = kwargs.get(f'{model_type}_model_name')
            model_cls = choices.get(name) if name is not None else flow_cls.get_default_models().get(model_type)
            if model_cls is None:
                raise ValueError(f'{flow_cls.__name__} has no {model_type} model named {name!r}')
            kwargs[f'{model_type}_model'] = model_cls(**{k: v for k, v in kwargs.items() if not k.endswith('_model')})
    flow = flow_cls(**kwargs)
    flow.load_state_dict(checkpoint['state_dict'], strict=True)
    if map_location is not None:
        flow.to(map_location)
    return flow
